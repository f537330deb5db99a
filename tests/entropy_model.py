"""A plain baseline-JPEG entropy coder of one scan, and a record of what it saw.  TEST INFRASTRUCTURE.

The coder takes the quantized zig-zag blocks of a picture in coding order (oracle.scan_coeffs), the sampling, and the
code words a caller hands to the library (dc_codes[2][12], ac_codes[2][256], each `code << 16 | length`).  It returns
the stuffed entropy-coded segment -- DC differences per component, run/size symbols with ZRL and EOB, packed MSB
first, FF -> FF 00, padded with 1-bits -- and a Trace of everything the kernels' table-dependent decisions hang on.

What the trace says about the library's work split is RESTATED here from DESIGN.md section 4 and the comments above
the walks, never imported from the library:
  * a segment is 41 / 82 / 246 consecutive MCUs (4:2:0 / 4:4:4 / 4:0:0): 246 coded blocks in every mode;
  * a block is coded as up to four parts, the quarters of its zig-zag scan (1-15 with the DC, 16-31, 32-47, 48-63;
    quarter 0 always makes a part, another quarter only when it holds a symbol); quarters 0 + 1 and 2 + 3 are ONE
    part when the block is lean, both quarters hold symbols, at most 16 between them, and fewer than 16 zeros lie
    between the last symbol of the first and the first symbol of the second;
  * n_safe of an AC table is the largest n (0..10) with len(0, n') + n' <= 16 for all 1 <= n' <= n; a block with an AC
    level of more than n_safe bits is checked, every other block lean;
  * only a part's first symbol can need ZRL codes, and never in quarter 0;
  * a checked part of more than 8 words takes a row of the frame's pool; the stitch window holds 1 112 words.
"""
import numpy as np

YUV_420, YUV_444, YUV_400 = 1, 3, 4
SEGMENT_MCUS = {YUV_420: 41, YUV_444: 82, YUV_400: 246}
# component of every block of an MCU; component 0 codes with table 0, the others with table 1
MCU_COMPONENTS = {YUV_420: (0, 0, 0, 0, 1, 2), YUV_444: (0, 1, 2), YUV_400: (0,)}
WINDOW_WORDS = 1112
ZRL, EOB = 0xF0, 0x00


# ---------------------------------------------------------------------------------------------- tables

def codes_from_lengths(lengths, size=256):
    """{symbol: length} -> (bits[16], syms, codes[size]): the JPEG table description (symbols by length, ascending
    within a length) and its canonical codes, `code << 16 | length` (0 = the symbol has no code).  The table must
    be a valid baseline table: lengths 1..16, Kraft sum below 1 -- so no code is all ones."""
    assert lengths and all(1 <= l <= 16 for l in lengths.values()) and all(0 <= s < size for s in lengths)
    kraft = sum(1 << (16 - l) for l in lengths.values())
    assert kraft < (1 << 16), "Kraft sum must stay below 1 (the all-ones code is reserved)"
    bits = np.zeros(16, np.uint8)
    syms = sorted(lengths, key=lambda s: (lengths[s], s))
    for s in syms:
        bits[lengths[s] - 1] += 1
    codes = np.zeros(size, np.uint32)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(int(bits[ln - 1])):
            assert code < (1 << ln) - 1
            codes[syms[k]] = (code << 16) | ln
            code += 1
            k += 1
        code <<= 1
    return bits, np.array(syms, np.uint8), codes


def lengths_of(codes):
    """{symbol: length} of a table of `code << 16 | length` words"""
    return {s: int(c) & 0xFF for s, c in enumerate(np.asarray(codes).reshape(-1)) if int(c) & 0xFF}


def description_of(codes):
    """(bits[16], syms) that rebuild `codes` canonically: symbols by (length, code)"""
    cs = [(int(c) & 0xFF, int(c) >> 16, s) for s, c in enumerate(np.asarray(codes).reshape(-1)) if int(c) & 0xFF]
    cs.sort()
    bits = np.zeros(16, np.uint8)
    for ln, _, _ in cs:
        bits[ln - 1] += 1
    return bits, np.array([s for _, _, s in cs], np.uint8)


def huffman_specs(sj, dc_codes, ac_codes):
    """The four HuffmanSpec (DC luma, DC chroma, AC luma, AC chroma) that make make_header_ex carry the tables"""
    specs = (sj.HuffmanSpec * 4)()
    for i, codes in enumerate((dc_codes[0], dc_codes[1], ac_codes[0], ac_codes[1])):
        bits, syms = description_of(codes)
        specs[i].bits[:] = [int(b) for b in bits]
        for k, s in enumerate(syms):
            specs[i].syms[k] = int(s)
        specs[i].nsyms = len(syms)
    return specs


def n_safe_of(ac_codes_one):
    """largest n with len(0, n') + n' <= 16 for all n' <= n (a missing code has length 0)"""
    n_safe = 0
    for n in range(1, 11):
        if (int(ac_codes_one[n]) & 0xFF) + n > 16:
            break
        n_safe = n
    return n_safe


# ---------------------------------------------------------------------------------------------- the coder

class Symbols:
    """What a scan is made of before any table is chosen: its items in coding order -- a DC size, a ZRL, a run/size
    symbol or an EOB, each with the bits that follow its code -- and what the blocks look like to the part rules."""

    def __init__(self, zz, yuv_mode):
        zz = np.asarray(zz)
        comps = MCU_COMPONENTS[yuv_mode]
        bpm = len(comps)
        assert zz.ndim == 2 and zz.shape[1] == 64 and zz.shape[0] % bpm == 0
        self.yuv_mode, self.nblocks = yuv_mode, zz.shape[0]
        self.seg_blocks = SEGMENT_MCUS[yuv_mode] * bpm
        blk, tbl, isdc, sym, extra, nextra, quarter, chain = [], [], [], [], [], [], [], []
        self.dc_signs = np.zeros((2, 12, 2), np.int64)
        self.first_of_quarter = [set(), set()]
        nb_ = self.nblocks
        self.block_table = np.zeros(nb_, np.int8)
        self.block_size = np.zeros(nb_, np.int8)           # bits of the block's largest AC level (0: none)
        self.cand01 = np.zeros(nb_, bool)                  # quarters 0 + 1 (2 + 3) make one part if the block is lean
        self.cand23 = np.zeros(nb_, bool)
        self.open1 = np.zeros(nb_, np.int16)               # the symbol that opens quarter 1 (3), -1: none
        self.open3 = np.zeros(nb_, np.int16)
        self.has_q = np.zeros((nb_, 4), bool)
        pred = [0, 0, 0]

        def item(b, t, d, s, e, n, q, c=0):
            blk.append(b); tbl.append(t); isdc.append(d); sym.append(s); extra.append(e); nextra.append(n)
            quarter.append(q); chain.append(c)

        for b, row in enumerate(zz.tolist()):
            comp = comps[b % bpm]
            t = 0 if comp == 0 else 1
            self.block_table[b] = t
            diff = row[0] - pred[comp]
            pred[comp] = row[0]
            n = abs(diff).bit_length()
            assert n <= 11, "DC difference out of baseline range"
            self.dc_signs[t][n][1 if diff < 0 else 0] += 1
            item(b, t, True, n, (diff - 1 if diff < 0 else diff) & ((1 << n) - 1), n, 0)
            nzpos = [i for i in range(1, 64) if row[i]]
            prev, maxsize = 0, 0
            opened = [-1, -1, -1, -1]
            for i in nzpos:
                v = row[i]
                run = i - prev - 1
                prev = i
                q = i >> 4
                for j in range(run >> 4):
                    item(b, t, False, ZRL, 0, 0, q, (run >> 4) if j == 0 else 0)
                n = abs(v).bit_length()
                assert n <= 10, "AC level out of baseline range"
                maxsize = max(maxsize, n)
                s = ((run & 15) << 4) | n
                if opened[q] < 0:
                    opened[q] = s
                    if q:
                        self.first_of_quarter[t].add((s, q))
                item(b, t, False, s, (v - 1 if v < 0 else v) & ((1 << n) - 1), n, q)
            if prev != 63:
                item(b, t, False, EOB, 0, 0, prev >> 4)
            self.block_size[b] = maxsize
            qp = [[i for i in nzpos if i >> 4 == q] for q in range(4)]
            end0 = (qp[0][-1] + 1) if qp[0] else 1         # position after the last non-zero of quarter 0 (1: none)
            end2 = (qp[2][-1] - 32 + 1) if qp[2] else 0    # the same of quarter 2, local (0: none)
            self.cand01[b] = bool(qp[1]) and (qp[1][0] - 16) < end0 and len(qp[0]) + len(qp[1]) <= 16
            self.cand23[b] = bool(qp[3]) and (qp[3][0] - 48) < end2 and len(qp[2]) + len(qp[3]) <= 16
            self.open1[b], self.open3[b] = opened[1], opened[3]
            self.has_q[b] = [True, bool(qp[1]), bool(qp[2]), bool(qp[3])]
        self.blk = np.array(blk, np.int64)
        self.tbl = np.array(tbl, np.int64)
        self.isdc = np.array(isdc, bool)
        self.sym = np.array(sym, np.int64)
        self.extra = np.array(extra, np.int64)
        self.nextra = np.array(nextra, np.int64)
        self.quarter = np.array(quarter, np.int64)
        self.chain = np.array(chain, np.int64)              # k on the first ZRL of a chain of k


class Trace:
    """what the coder saw under one set of tables (arrays by block, by part, by segment)"""

    def stats(self):
        """the counts as oracle.symbol_stats lays them out: [2][272], 256 AC then 16 DC"""
        f = np.zeros((2, 272), np.int64)
        f[:, :256] = self.ac_counts
        f[:, 256:268] = self.dc_counts
        return f

    def segment_words(self):
        return [(int(b) + 31) // 32 for b in self.segment_bits]


def encode_symbols(S, dc_codes, ac_codes):
    """Symbols -> (stuffed bytes, Trace) under the given code words"""
    dc = np.asarray(dc_codes, np.int64).reshape(2, 12)
    ac = np.asarray(ac_codes, np.int64).reshape(2, 256)
    code = np.where(S.isdc, dc[S.tbl, np.minimum(S.sym, 11)], ac[S.tbl, S.sym])
    ln = code & 0xFF
    assert (ln > 0).all(), "a symbol of this picture has no code in the table"
    val = ((code >> 16) << S.nextra) | S.extra
    nb = ln + S.nextra
    end = np.cumsum(nb)
    start = end - nb
    total = int(end[-1])
    # MSB-first packing: an item has at most 27 bits and starts at bit (start mod 32) of a word, so it lies inside the
    # 64 bits of that word and the next; no two items share a bit, so adding is ORing (and exact in float64: < 2^32)
    nwords = (total + 31) // 32 + 1
    w64 = val << (64 - (start & 31) - nb)
    words = (np.bincount(start >> 5, weights=(w64 >> 32) & 0xFFFFFFFF, minlength=nwords)
             + np.bincount((start >> 5) + 1, weights=w64 & 0xFFFFFFFF, minlength=nwords + 1)[:nwords])
    raw = bytearray(words.astype(np.uint64).astype(">u4").tobytes()[:(total + 7) // 8])
    if total & 7:
        raw[-1] |= (1 << (8 - (total & 7))) - 1            # padded with 1-bits
    tr = Trace()
    tr.total_bits = total
    tr.unstuffed_len = len(raw)
    tr.ff_bytes = raw.count(0xFF)
    # what a bit counter reports: the bits, and 8 more for every 0xFF among the COMPLETED bytes (the padding completes none)
    tr.counted_bits = total + 8 * bytes(raw[:total // 8]).count(0xFF)
    stuffed = bytes(raw).replace(b"\xff", b"\xff\x00")
    tr.stuffed_len = len(stuffed)
    # ---- the trace
    nblk = S.nblocks
    tr.ac_counts = np.bincount((S.tbl * 256 + S.sym)[~S.isdc], minlength=512).reshape(2, 256)
    tr.dc_counts = np.bincount((S.tbl * 12 + S.sym)[S.isdc], minlength=24).reshape(2, 12)
    tr.dc_signs = S.dc_signs
    tr.first_of_quarter = S.first_of_quarter
    tr.n_safe = (n_safe_of(ac[0]), n_safe_of(ac[1]))
    tr.block_table, tr.block_size = S.block_table, S.block_size
    tr.block_bits = np.bincount(S.blk, weights=nb, minlength=nblk).astype(np.int64)
    tr.block_checked = S.block_size > np.array(tr.n_safe)[S.block_table]
    seg_of_item = S.blk // S.seg_blocks
    tr.segment_bits = np.bincount(seg_of_item, weights=nb).astype(np.int64)
    seg_start = np.concatenate(([0], np.cumsum(tr.segment_bits)[:-1]))
    # parts: a checked block merges nothing
    m01, m23 = S.cand01 & ~tr.block_checked, S.cand23 & ~tr.block_checked
    tr.first_of_merged = [set(), set()]
    for t in range(2):
        mine = S.block_table == t
        tr.first_of_merged[t] = set(S.open1[m01 & mine].tolist()) | set(S.open3[m23 & mine].tolist())
    q = S.quarter.copy()
    q[(q == 1) & m01[S.blk]] = 0
    q[(q == 3) & m23[S.blk]] = 2
    key = S.blk * 4 + q
    bits_by = np.bincount(key, weights=nb, minlength=4 * nblk).astype(np.int64).reshape(nblk, 4)
    regular = ~S.isdc & (S.sym != ZRL) & (S.sym != EOB)
    syms_by = np.bincount(key[regular], minlength=4 * nblk).reshape(nblk, 4)
    exists = S.has_q.copy()
    exists[:, 1] &= ~m01
    exists[:, 3] &= ~m23
    pb, pq = np.nonzero(exists)
    tr.part_block, tr.part_quarter = pb, pq
    tr.part_merged = ((pq == 0) & m01[pb]) | ((pq == 2) & m23[pb])
    tr.part_checked = tr.block_checked[pb]
    tr.part_symbols, tr.part_bits = syms_by[pb, pq], bits_by[pb, pq]
    assert int(bits_by.sum()) == int(tr.part_bits.sum()) == total
    # ZRL chains: (table, k, zl, start bit in its segment mod 32, quarter of the symbol behind)
    heads = np.nonzero(S.chain)[0]
    offs = (start[heads] - seg_start[seg_of_item[heads]]) & 31
    tr.zrl_chains = list(zip(S.tbl[heads].tolist(), S.chain[heads].tolist(), ln[heads].tolist(), offs.tolist(),
                             S.quarter[heads].tolist()))
    return stuffed, tr


def encode_scan(zz, yuv_mode, dc_codes, ac_codes):
    """zz: int16 [blocks][64] in coding order.  Returns (stuffed bytes, Trace)."""
    return encode_symbols(Symbols(zz, yuv_mode), dc_codes, ac_codes)


def scan_body(jpeg):
    """the entropy-coded segment of a baseline JPEG with one scan: what lies behind the SOS header and in front of EOI"""
    jpeg = bytes(jpeg)
    i = 2
    while True:
        assert jpeg[i] == 0xFF
        marker = jpeg[i + 1]
        n = (jpeg[i + 2] << 8) | jpeg[i + 3]
        i += 2 + n
        if marker == 0xDA:
            break
    assert jpeg[-2:] == b"\xff\xd9"
    return jpeg[i:-2]


MAX_BLOCK_BITS = 1728            # what a segment's worst-case slot allows per block


def slot_words(capacity_bytes, nseg):
    """words of a segment's slot when a frame may take capacity_bytes: three quarters of the
    segment's share of the budget, in units of 64 words, at least 1 024 and at most the worst case"""
    worst = ((246 * MAX_BLOCK_BITS + 31) // 32 + 2 + 3) & ~3
    budget = min(capacity_bytes // 4 + 16, nseg * worst)
    sw = (budget * 3 // nseg // 4 + 63) & ~63
    sw = max(sw, min(worst, 1024))
    if sw > worst or budget >= nseg * worst:
        sw = worst
    return sw
