"""CPU half of the directed stitch tests: the plain stitch of tests/stitch_model.py is pinned on the oracle, the ruler
pictures of tests/stitch_cases.py on the entropy model, and the coverage of every route is asserted on the model's
events alone.  tests/test_stitch_directed.py (GPU) runs exactly the cases counted here.

Places a route cannot reach are listed by name in UNREACHABLE, with the reason."""
import functools
from collections import Counter

import numpy as np
import pytest

import entropy_model as em
import stitch_cases as sc
import stitch_model as sm
from oracle import synth

# ---------------------------------------------------------------------------------------------- what must be reached

K5_PAIRS = [f"K5 group: ff@{j} behind {s}" for j in range(16) for s in ("plain", "ff@0", "ff@1", "ff@2", "ff@3")]
K5_BANDS = (K5_PAIRS
            + [f"K5 group: plain behind ff@{b} ({'fast' if b == 3 else 'slow'})" for b in range(4)]
            + ["K5 group: fast", "K5 group: slow", "K5 slow thread in front of a fast one", "K5 fast thread in front of a slow one",
               "K5 last thread of a chunk slow by the next chunk's first bytes",
               "K5 FF is the last byte of a full chunk", "K5 FF is the first byte of a chunk behind the first", "K5 chunk of 4096 FF"]
            + [f"K5 run of {n} FF {'at' if n == 1 else 'across'} a {u} boundary" for n in range(1, 6) for u in ("group", "chunk")]
            + [f"K5 last thread has {v} bytes" for v in range(1, 16)]
            + [f"K5 U = {u}" for u in range(1, 18)] + ["K5 U = 4096 k", "K5 U = 4096 k + 1", "K5 U = 4096 k - 1"]
            + ["K5 copy-out byte by byte (no aligned 16 inside)"]
            + [f"K5 mis = {m} (later chunk)" for m in range(16)] + [f"K5 mis = {m} (first chunk)" for m in range(16)]
            + [f"K5 T mod 8 = {r}: the padded last byte is {w}" for r in range(1, 8) for w in ("FF", "not FF")]
            + ["K5 T mod 8 = 0: the last byte is FF", "K5 T mod 8 = 0: the last byte is not FF"]
            + ["K5 chunk offset from co[] (K4)", "K5 a workgroup takes a second chunk"])
K3_BANDS = ([f"K3 lead = {v}" for v in range(32)] + [f"K3 edge word holds {v} bits of its segment" for v in range(1, 32)]
            + ["K3 edge_easy false: the segment behind is shorter than what the word lacks",
               "K3 edge word finished from three or more segments", "K3 FF byte made of bits of two segments",
               "K3 empty segment", "K3 empty segments follow each other", "K3 few-bit segments follow each other",
               "K3 segment starts no word of its own"]
            + [f"K3 edge_valid = {v} in an earlier segment's word" for v in (1, 2, 3, 4)] + [f"K3 edge_valid = {v}" for v in (1, 2, 3, 4)]
            + [f"K3 FF at byte {b} of an edge word" for b in range(4)]
            + [f"K3 FF in the frame's last word, edge_valid = {v}" for v in (1, 2, 3)]
            + ["K3 a wave's 64 words straddle a chunk boundary", "K3 wave straddles a chunk boundary with FF behind it",
               "K3 wave straddles a chunk boundary with FF in front of it",
               "K3 band of exactly 32 * stride bits", "K3 band of 32 * stride - 1 bits", "K3 subs = 1", "K3 subs > 1",
               "K3 stride < 768", "K3 stride 769..775", "K3 stride >= 776",
               "K3 segment longer than one wave's 768 speculative words", "K3 segment longer than 1024 words",
               "K3 segment placed by the narrow path", "K3 segment placed by the long (slot/pool mapping) path"])
K24_BANDS = ["K2 scan kernel", "K2 clears the chunks' 0xFF counters", "K2 second round of 2048 segments",
             "K2 two-halves scan: a round's total passes 2^24", "K2 two-halves scan: a thread's run passes 2^24",
             "K4 scan kernel", "K4 second round of 2048 chunks"]

# the wide form of K3, whatever kernel holds the scans: what the ruler pictures must reach in EVERY picture route
K3_WIDE = ([f"K3 lead = {v}" for v in range(0, 32, 2)] + [f"K3 edge word holds {v} bits of its segment" for v in range(2, 32, 2)]
           + ["K3 edge_easy false: the segment behind is shorter than what the word lacks", "K3 segment starts no word of its own"]
           + [f"K3 edge_valid = {v} in an earlier segment's word" for v in (1, 2, 3, 4)] + ["K3 edge_valid = 4"]
           + [f"K3 FF at byte {b} of an edge word" for b in range(4)]
           + [f"K3 FF in the frame's last word, edge_valid = {v}" for v in (1, 2, 3)]
           + [f"K3 a lane's four words straddle a chunk boundary, wbeg mod 4 = {m}" for m in (1, 2, 3)]
           + ["K3 lane straddles a chunk boundary with FF in front of it", "K3 lane straddles a chunk boundary with FF behind it",
              "K3 segment longer than one wave's 768 speculative words", "K3 segment longer than 1024 words",
              "K3 segment placed by the wide path", "K3 FF byte made of bits of two segments"])
K5_PICTURES = ["K5 group: fast", "K5 group: slow", "K5 slow thread in front of a fast one", "K5 fast thread in front of a slow one",
               "K5 FF is the last byte of a full chunk", "K5 FF is the first byte of a chunk behind the first",
               "K5 T mod 8 = 0: the last byte is not FF"] + [f"K5 T mod 8 = {r}: the padded last byte is not FF" for r in (2, 4, 6)] + [
                   "K5 T mod 8 = 1: the padded last byte is FF"]
POOL = ["K3 segment longer than its slot", "K3 segment placed by the long (slot/pool mapping) path"]

REQUIRED = {
    "bands": K5_BANDS + K3_BANDS + K24_BANDS,
    "fused 1, tight": K3_WIDE + K5_PICTURES + POOL + ["K3 wide_subs: sub-ranges of 768 words", "K2 inside K3: whole scan in LDS",
                                                      "K5 chunk offset from fused_off[] (LDS)"],
    "fused 1": K3_WIDE + K5_PICTURES + ["K3 wide_subs: sub-ranges of 768 words", "K2 inside K3: whole scan in LDS",
                                        "K5 chunk offset from fused_off[] (LDS)"],
    "fused 2": K3_WIDE + K5_PICTURES + ["K3 wide_subs: sub-ranges of 768 words", "K2 inside K3: window of eight, sums on demand",
                                        "K5 chunk offset from big_off (sums on demand)"],
    "packed, 4 frames": K3_WIDE + K5_PICTURES + ["K2 scan kernel", "K4 scan kernel", "K5 chunk offset from co[] (K4)"],
    "per-frame tables, 3 frames": K3_WIDE + K5_PICTURES + ["K2 inside K3: whole scan in LDS", "K5 chunk offset from fused_off[] (LDS)"],
    "ragged": K3_WIDE + K5_PICTURES + POOL + ["K2 scan kernel", "K4 scan kernel", "K5 chunk offset from co[] (K4)"],
    "restart": ["K6 placeholder at chunk byte 4095", "K6 several FF in front of the marker in its chunk",
                "K6 placeholder straddles a chunk boundary with FF in front of it", "K6 placeholder inside a chunk",
                "K2 scan kernel", "K4 scan kernel"],
    "64 frames": ["K5 a workgroup takes a second chunk", "K5 chunk offset from co[] (K4)"],
}

_EVEN = "every block of a ruler starts at an even bit, so a segment does too: bands reach the odd values"
UNREACHABLE = {
    "every picture route": {
        "K3 lead / edge bits odd": _EVEN,
        "K5 padded last byte FF at T mod 8 other than 1": "the flat pictures' blocks end in `01`: one real 1-bit in the last byte; "
                                                          "bands, every T mod 8",
        "K3 edge word holds 0 bits of its segment": "a segment that ends on a word boundary has no edge word: the word behind "
                                                    "is the next segment's first (any route)",
        "K3 edge_valid = 0": "a word that starts at or behind the stream's end is no destination word of any segment: "
                             "the branch that uses edge_valid is not taken (any route)",
        "K5 every (position, group behind) pair, runs, U = 1..17, every mis": "K5's byte logic is one code in every form: bands",
        "K3 empty segment": "a segment of a picture holds at least one block: 2 bits",
        "K2 / K4 second round": "more than 2048 segments or chunks in a picture: the existing 8K digest test; bands here",
    },
    "fused 2": {"(which pictures)": "form 2 needs 158 segments: the main ruler and sc.big_rulers() alone go through it",
                "K3 segment longer than its slot": "a slot shorter than a segment needs a small capacity, form 2 more than 2048 "
                                                   "chunks of scratch",
                "K5 big_off stepping to a workgroup's second chunk": "a frame above 4096 chunks: stays with the 8K digest test",
                "K3 off() walking past the window of eight": "eight segments in a row that start no word: a picture has one "
                                                             "short segment, its last"},
    "fused 1": {"K3 segment longer than its slot": "at 1 MiB a slot holds the longest segment: the tight capacity reaches it"},
    "packed, 4 frames": {"K3 segment longer than its slot": "as fused 1"},
    "per-frame tables, 3 frames": {"K3 segment longer than its slot": "as fused 1"},
    "bands": {"K3 segment longer than its slot": "bands have no pool: a band is at most its stride",
              "K3 lane straddle (wide form)": "bands take the narrow form: one word a lane",
              "fused forms, K6": "the band entry launches K2..K5 as kernels, without markers"},
}


@functools.lru_cache(maxsize=None)
def _modelled(name, oracle):
    """(picture, segment bits, un-stuffed bytes, stuffed body) of a ruler picture under the ruler's tables"""
    pic = next(p for p in sc.pictures() if p.name == name)
    case = pic.case(oracle)
    body, tr = em.encode_symbols(case.symbols(oracle), *pic.codes())
    return pic, tr.segment_bits, body.replace(b"\xff\x00", b"\xff"), body


def _ff(raw):
    return np.nonzero(np.frombuffer(raw, np.uint8) == 0xFF)[0].tolist()


# ---------------------------------------------------------------------------------------------- the model

def test_stitch_of_the_oracles_bits_is_the_oracles_stream(oracle):
    for (w, h, q, mode, noise) in ((200, 120, 80.0, 1, False), (64, 64, 98.0, 3, True), (333, 211, 40.0, 4, False),
                                   (97, 61, 100.0, 1, True), (640, 360, 92.0, 3, True)):
        img = synth.g_noise(w, h, 9) if noise else synth.g_struct(w, h, 9)
        qm = oracle.quality_matrices(q)
        zz = oracle.scan_coeffs(img, qm, yuv_mode=mode)
        body, tr = em.encode_scan(zz, mode, *oracle.default_codes())
        bits = np.unpackbits(np.frombuffer(body.replace(b"\xff\x00", b"\xff"), np.uint8))[:tr.total_bits]
        edges = np.concatenate(([0], np.cumsum(tr.segment_bits)))
        strings = [bits[edges[i]:edges[i + 1]] for i in range(len(tr.segment_bits))]
        header = oracle.headers(w, h, mode, qm)
        assert sm.stitch(strings, header, True) == oracle.encode_matrices(img, qm, yuv_mode=mode), (w, h, q, mode)
        assert sm.stitch(strings, b"", False) == bytes(oracle.scan_bits(img, qm, yuv_mode=mode))
        # words and back
        assert all((sm.bits_of(sm.words_of(s), len(s)) == s).all() for s in strings)


def test_restart_form_is_the_oracles(oracle):
    import sjpeg_amd as sj
    for (w, h, q, mode) in ((333, 211, 75.0, 1), (300, 260, 50.0, 4), (200, 120, 90.0, 3), (16 * 41 + 1, 16, 60.0, 1)):
        img = synth.g_struct(w, h, 5 + w)
        zz = oracle.scan_coeffs(img, oracle.quality_matrices(q), yuv_mode=mode)
        body, raws = sm.encode_restart(zz, mode, *oracle.default_codes())
        assert em.scan_body(oracle.encode_rst(img, q, mode, sj.restart_interval(mode))) == body, (w, h, q, mode)
        seg, raw = sm.restart_stream(raws)
        assert int(seg.sum()) == 8 * len(raw)


def test_forms_are_the_expected_ones():
    main = sc.rulers()[0]
    assert main.nseg == 201 >= 158
    want = {"fused 1, tight": (1, 1), "fused 1": (1, 1), "fused 2": (2, 2), "packed, 4 frames": (0, 0),
            "per-frame tables, 3 frames": (1, 1)}
    for route, (stride, form) in sc.uniform_routes(main, 13000, 330).items():
        assert (form["fused_k2"], form["fused_k4"]) == want[route], route
        assert form["wide"] and form["wide_subs"] and stride % 16 == 0
    assert sm.uniform_form(1, 201, sc.FUSED1_STRIDE, restart=True)["fused_k4"] == 0
    f = sm.uniform_form(64, 16, 1 << 20, packed=True)
    assert f["gx"] == 64 and f["fused_k4"] == 0
    f = sm.ragged_form([4096] * 63 + [1 << 20], [1] * 63 + [16], 63)
    assert f["gx"] == 64 and f["subs"] == 1 and f["wide"]
    b = sc.big_band_case().form()
    assert b["gx"] == 4096 and b["subs"] > 1


# ---------------------------------------------------------------------------------------------- the rulers

@pytest.mark.parametrize("name", [p.name for p in sc.rulers() + sc.tail_rulers() + sc.flat_rulers() + sc.big_rulers()[:-1]])
def test_ruler_has_its_ff_bytes_where_they_were_designed(oracle, name):
    pic, seg, raw, _ = _modelled(name, oracle)
    d_seg, d_raw = pic.design()
    assert (seg == d_seg).all() and raw == d_raw, name
    assert _ff(raw) == sorted(pic.targets()), name


@pytest.mark.parametrize("name", [p.name for p in sc.dense_rulers() + sc.big_rulers()[-1:]])
def test_dense_ruler_has_its_ff_bytes_where_they_were_designed(oracle, name):
    pic, seg, raw, _ = _modelled(name, oracle)
    first = (pic.ruler_from + 7) // 8
    assert [f for f in _ff(raw) if f >= first] == pic.targets(), name
    assert len(_ff(raw[:first])) >= 8                       # the prefix: noise, 0xFF where chance puts it
    words = (seg + 31) // 32
    assert words[-1] < 64 and (words[:-1] > 768).sum() >= 1


def test_dense_rulers_make_the_long_segments(oracle):
    by = {n: (_modelled(n, oracle)[1] + 31) // 32 for n in ("dense-ruler-768", "dense-ruler-1024", "dense-ruler-pool")}
    assert 768 < by["dense-ruler-768"][0] <= 1024 < by["dense-ruler-1024"][0]
    assert (by["dense-ruler-pool"][:2] > 1152).all()


def test_main_ruler_is_the_one_described():
    main = sc.rulers()[0]
    assert (main.w, main.h, main.n, main.nseg) == (1792, 1760, 49280, 201)
    assert main.targets() == [8, 4095, 4100, 8192, 12287]


def test_restart_ruler_is_what_the_model_codes(oracle):
    r = sc.restart_ruler()
    case = r.case()
    _, raws = sm.encode_restart(case.coeffs(oracle), em.YUV_400, *sc.ruler_codes())
    assert raws == r.restart_design()


def test_saturated_noise_has_66_chunks(oracle):
    c = sc.saturated_noise()
    _, tr = em.encode_symbols(c.symbols(oracle), *oracle.default_codes())
    assert tr.unstuffed_len >= 66 * sm.CHUNK
    assert tr.unstuffed_len <= 128 * sm.CHUNK               # (two chunks a workgroup of 64, not three)


def test_band_cases_stitch_to_their_streams():
    for c in sc.band_cases():
        raw, total = sm.raw_stream(c.bands())
        assert total == c.total_bits and len(raw) == (total + 7) // 8
        w = c.words()
        assert all((sm.bits_of(w[i], n) == b).all() for i, (n, b) in enumerate(zip(c.lens, c.bands())))


# ---------------------------------------------------------------------------------------------- coverage

def route_events(oracle):
    """route -> Counter of the events its cases reach (what the GPU file runs, case for case)"""
    import sjpeg_amd as sj
    out = {r: Counter() for r in REQUIRED}
    for c in sc.band_cases() + [sc.big_band_case()]:
        raw, _ = sm.raw_stream(c.bands()) if c.name != "17MB" else (bytes(c._raw[:-1]) + bytes([c._raw[-1] | 7]), 0)
        out["bands"].update(sm.events(np.array(c.lens, np.int64), raw, len(c.header), c.form()))
    pics = [_modelled(p.name, oracle) for p in sc.pictures()]
    hlen = {}
    for pic, seg, raw, body in pics:
        case = pic.case(oracle)
        hlen[pic.name] = len(sj.make_header_ex(pic.w, pic.h, em.YUV_400, case.quant, em.huffman_specs(sj, *pic.codes())))
        for route, (stride, form) in sc.uniform_routes(pic, hlen[pic.name] + len(body) + 2, hlen[pic.name]).items():
            out[route].update(sm.events(seg, raw, hlen[pic.name], form))
    caps = [sc.tight(hlen[p.name] + len(body) + 2) for p, _, _, body in pics]
    for k, (pic, seg, raw, body) in enumerate(pics):
        out["ragged"].update(sm.events(seg, raw, hlen[pic.name], sm.ragged_form(caps, [p.nseg for p, _, _, _ in pics], k)))
    r = sc.restart_ruler()
    seg, raw = sm.restart_stream(r.restart_design())
    out["restart"].update(sm.events(seg, raw, 0, sm.uniform_form(1, r.nseg, sc.FUSED1_STRIDE, restart=True)))
    c = sc.saturated_noise()
    body, tr = em.encode_symbols(c.symbols(oracle), *oracle.default_codes())
    out["64 frames"].update(sm.events(tr.segment_bits, body.replace(b"\xff\x00", b"\xff"), 0,
                                      sm.uniform_form(64, len(tr.segment_bits), 1 << 20, packed=True)))
    return out


def test_every_place_is_reached_in_every_route_that_can_reach_it(oracle):
    got = route_events(oracle)
    missing = {route: [e for e in REQUIRED[route] if got[route][e] == 0] for route in REQUIRED}
    assert not any(missing.values()), {r: m for r, m in missing.items() if m}
