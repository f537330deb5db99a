"""Inputs of the directed stitch tests: bit strings for the band entry with a 0xFF at every designed place, and "ruler"
pictures that put a 0xFF at chosen bytes of the un-stuffed stream of an ORDINARY encode.  TEST INFRASTRUCTURE.

The ruler.  A gray picture with DC step 1 and large AC steps, coded with DC lengths {size 0: 1, size 10: 2, the rest
3..12} (canonical: `0` for size 0, `10` for size 10) and the `eob:1` AC family (EOB = `0`):
  * a block whose DC level does not move costs 2 bits, `00`;
  * the step -511 -> 512 costs 13 bits, `10` + ten 1-bits + `0`; the step back 13 bits with ten 0-bits;
  * the picture starts with the levels -512, -511: 13 + 5 = 18 bits, so that every block starts at an even bit.
An up-step whose ten 1-bits begin at bit 8 t makes byte t of the stream an isolated 0xFF; an up-step whose 1-bits begin
at a bit = 2 or 4 (mod 8) makes none, and only moves everything behind it by 26 - 4 = 22 bits: that is how a segment's
first word, its `lead` and the frame's last byte are steered.  What a ruler really holds is what the oracle's
coefficients give under the model (tests/test_stitch_model_host.py pins every ruler's 0xFF positions on it); the
design below works on the same arithmetic written out, so that a search over designs costs milliseconds.
"""
import functools

import numpy as np

import entropy_cases as ec
import entropy_model as em
import stitch_model as sm

SEG_BLOCKS = 246                                           # 4:0:0
RULER_DC = {0: 1, 10: 2, 1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 6: 8, 7: 9, 8: 10, 9: 11, 11: 12}


@functools.lru_cache(maxsize=None)
def ruler_codes():
    """(dc_codes[2][12], ac_codes[2][256]) of the ruler; a gray picture codes with table 0 alone"""
    dc = em.codes_from_lengths(RULER_DC, 12)[2]
    ac = em.codes_from_lengths(ec.ac_family("eob:1"), 256)[2]
    return np.stack([dc, dc]), np.stack([ac, ac])


# ---------------------------------------------------------------------------------------------- band cases

class BandCase:
    def __init__(self, name, raw, total_bits, lens, stride=None, header=b""):
        """raw: the un-stuffed bytes (the last one's padding whatever); lens: the bands' bit lengths"""
        assert sum(lens) == total_bits and (total_bits + 7) // 8 == len(raw)
        self.name, self.header, self.lens = name, header, [int(v) for v in lens]
        self.total_bits = total_bits
        need = max(4, max((v + 31) // 32 for v in lens))
        self.stride = need if stride is None else stride
        assert self.stride >= need
        self._raw = np.frombuffer(bytes(raw), np.uint8)

    def bands(self):
        bits = np.unpackbits(self._raw)[:self.total_bits]
        edges = np.concatenate(([0], np.cumsum(self.lens)))
        return [bits[edges[i]:edges[i + 1]] for i in range(len(self.lens))]

    def words(self):
        """[nbands][stride] int32: what the band entry takes (bits behind a band's end: zero)"""
        out = np.zeros((len(self.lens), self.stride), np.int32)
        for i, b in enumerate(self.bands()):
            out[i] = sm.words_of(b, self.stride)
        return out

    def form(self):
        return sm.band_form(len(self.lens), self.stride)

    def __repr__(self):
        return self.name


def _plain(rs, n):
    return rs.randint(0, 255, n).astype(np.uint8)          # 0 .. 254: no 0xFF but the designed ones


def _cuts(rs, total, n):
    c = np.sort(rs.randint(0, total + 1, n - 1))
    e = np.concatenate(([0], c, [total]))
    return np.diff(e).tolist()


def _pairs_stream(rs):
    """every (position of an FF in a group) x (the group behind: plain, FF at byte 0, 1, 2 or 3 only), and a plain
    group in front of each such group behind -- once in chunk 0, once in chunk 1 one group later"""
    raw = _plain(rs, 2 * sm.CHUNK + 5)
    for base in (1, 256 + 2):
        g = base
        for j in range(16):
            for state in (-1, 0, 1, 2, 3):
                raw[16 * g + j] = 0xFF
                if state >= 0:
                    raw[16 * (g + 1) + state] = 0xFF
                g += 3
            if j % 4 == 3:                                 # four groups with no FF of their own, behind: FF at byte j // 4
                raw[16 * (g + 1) + j // 4] = 0xFF
                g += 3 if j < 15 else 0
        assert g < base + 253
    return raw


def _runs_stream(rs):
    """runs of 1..5 FF bytes lying across group boundaries (inside chunks) and across chunk boundaries, at every split"""
    splits = [(n, k) for n in range(1, 6) for k in (range(0, 2) if n == 1 else range(1, n))]   # k bytes in front of the boundary
    raw = _plain(rs, (len(splits) + 1) * sm.CHUNK + 77)
    for i, (n, k) in enumerate(splits):
        cb = (i + 1) * sm.CHUNK                            # a chunk boundary
        raw[cb - k:cb - k + n] = 0xFF
        gb = cb - 2048 + 16 * (i % 7)                      # a group boundary inside the chunk in front
        raw[gb - k:gb - k + n] = 0xFF
    return raw


@functools.lru_cache(maxsize=None)
def band_cases():
    rs = np.random.RandomState(20241019)
    out = []
    # --- K5, byte by byte
    pairs = _pairs_stream(rs)
    for h in range(16):                                    # ... at every misalignment of chunk 1 and 2
        out.append(BandCase(f"pairs-header{h + 16 * (h % 3)}", pairs, 8 * len(pairs), _cuts(rs, 8 * len(pairs), 6),
                            header=bytes(_plain(rs, h + 16 * (h % 3)))))
    runs = _runs_stream(rs)
    out.append(BandCase("runs", runs, 8 * len(runs), _cuts(rs, 8 * len(runs), 9), header=b"\xff\xd8HDR"))
    full = _plain(rs, 3 * sm.CHUNK + 100)
    full[sm.CHUNK:2 * sm.CHUNK] = 0xFF
    out.append(BandCase("chunk-of-ff", full, 8 * len(full), _cuts(rs, 8 * len(full), 4), header=b"H" * 7))
    allff = np.full(2 * sm.CHUNK, 0xFF, np.uint8)
    out.append(BandCase("two-chunks-of-ff", allff, 8 * len(allff), _cuts(rs, 8 * len(allff), 3)))
    # --- stream lengths and the last byte: T = 8 U - r, the last real bits ones (the padding makes the byte FF) or zeros
    for U in list(range(1, 18)) + [4095, 4096, 4097, 8192]:
        for r in (range(8) if U > 17 else ((U - 1) % 8, (U + 3) % 8)):
            for tail_ones in (True, False):
                raw = _plain(rs, U)
                if U > 100:
                    raw[rs.randint(0, U - 1, 24)] = 0xFF
                raw[-1] = 0xFF if tail_ones else int(raw[-1]) & 0x7F & (0xFF << r) & 0xFF
                if U > 1:
                    raw[-2] = 0xFF if (U + r) % 3 == 0 else raw[-2]
                T = 8 * U - r
                lens = _cuts(rs, T, 3 if U < 100 else 5)
                out.append(BandCase(f"U{U}-r{r}-{'ones' if tail_ones else 'zeros'}", raw, T, lens,
                                    header=bytes(_plain(rs, (U + r) % 16))))
    # --- K3: short and empty bands, edge words finished from many bands
    raw = _plain(rs, 700)
    raw[[3, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 40, 41, 42, 43, 699]] = 0xFF
    lens = [100, 0, 0, 0, 1, 31, 32, 33, 5, 7, 9, 0, 0, 11, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 64, 63, 65, 0, 1, 1, 1]
    lens += [8 * 700 - 4 - sum(lens) - 6, 1, 2, 3, 0, 0]
    out.append(BandCase("short-and-empty-bands", raw, 8 * 700 - 4, lens))
    for lead in range(32):                                 # every `lead`, every count of bits in the edge word
        raw = _plain(rs, 64)
        raw[[7, 8, 30, 31, 32, 33, 63]] = 0xFF
        lens = [32 - lead if lead else 32, 97 + lead, 200 - 3 * lead, 512 - (32 - lead if lead else 32) - (97 + lead) - (200 - 3 * lead)]
        out.append(BandCase(f"lead{lead}", raw, 512, lens))
    # --- K3: bands as long as their slot, strides on both sides of the narrow form's 768 words per wave
    for stride in (8, 767, 768, 770, 775, 776, 800, 1600, 2308):
        n = 4 * stride
        raw = _plain(rs, 3 * n + 9)
        raw[rs.randint(0, len(raw), len(raw) // 100)] = 0xFF
        raw[[n - 1, n, 2 * n - 1, 2 * n]] = 0xFF           # around the ends of the two full bands
        lens = [32 * stride, 32 * stride - 1, 32 * stride - 7, 80]
        out.append(BandCase(f"full-bands-stride{stride}", raw, sum(lens), lens, stride=stride, header=b"ab"))
    # --- K2: a second round of 2048 bands, totals past 2^24
    nb = 2100
    T = (1 << 24) + 12345
    raw = rs.randint(0, 256, (T + 7) // 8).astype(np.uint8)
    lens = np.full(nb, T // nb, np.int64)
    lens[:T % nb] += 1
    lens[5::97] -= 1
    lens[6::97] += 1
    lens[300] += lens[301]
    lens[301] = 0
    out.append(BandCase("2100-bands", raw, T, lens.tolist(), header=b"x" * 9))
    T = 10 * ((1 << 21) + 999) + 3
    raw = rs.randint(0, 256, (T + 7) // 8).astype(np.uint8)
    out.append(BandCase("ten-bands-of-2^21-bits", raw, T, [(1 << 21) + 999] * 9 + [(1 << 21) + 1002]))
    return out


@functools.lru_cache(maxsize=None)
def big_band_case():
    """more than 4096 chunks: a workgroup of the band entry takes a second chunk (natural 0xFF density, and designed ones
    around chunk 4096)"""
    rs = np.random.RandomState(4097)
    U = 4100 * sm.CHUNK + 1234
    raw = rs.randint(0, 256, U, dtype=np.uint8)
    b = 4096 * sm.CHUNK
    raw[b - 2:b + 3] = 0xFF
    raw[b + sm.CHUNK - 1] = 0xFF
    lens = [8 * (U // 9) + 5] * 8
    lens.append(8 * U - 3 - sum(lens))
    return BandCase("17MB", raw, 8 * U - 3, lens)


# ---------------------------------------------------------------------------------------------- rulers

class Ruler:
    """pairs: the even bit positions at which an up-step block starts (its ten 1-bits begin two bits on); the step back
    follows at once."""

    def __init__(self, name, blocks_w, blocks_h, pairs, end_up=False, no_eob_at=None):
        self.name, self.bw, self.bh = name, blocks_w, blocks_h
        self.pairs = sorted(int(p) for p in pairs)
        # block no_eob_at holds level 255 at zig-zag 63 and nothing else: `0`, three ZRL, (14, 8), eight 1-bits, NO EOB --
        # 45 bits that end in 1-bits; the block behind it steps up (`10` ...), the next one back
        self.no_eob_at = no_eob_at
        self._case = None
        self.end_up = end_up                               # the LAST block steps up, nothing steps back: the stream ends 11 bits on
        self.n = blocks_w * blocks_h
        self.w, self.h = 8 * blocks_w, 8 * blocks_h
        self.nseg = -(-self.n // SEG_BLOCKS)
        self._layout()

    def _layout(self):
        kinds = [3, 4]                                     # 0 plain, 1 up, 2 down, 3 / 4 the two head blocks, 6 without EOB
        pos = 18
        for p in self.pairs:
            assert p >= pos and (p - pos) % 2 == 0, (self.name, p, pos)
            kinds += [0] * ((p - pos) // 2) + [1, 2]
            pos = p + 26
        assert len(kinds) <= self.n, (self.name, "the design needs more blocks than the picture has")
        kinds += [0] * (self.n - len(kinds))
        self.kinds = np.array(kinds, np.int8)
        if self.no_eob_at is not None:
            k = self.no_eob_at
            assert (self.kinds[k:k + 3] == 0).all() and k + 3 <= self.n
            self.kinds[k:k + 3] = (6, 1, 2)
        if self.end_up:
            assert self.kinds[-1] == 0 and self.kinds[-2] != 1
            self.kinds[-1] = 1

    def levels(self):
        return np.array([-511, 512, -511, -512, -511, 0, -511])[self.kinds]

    def _no_eob_pattern(self):
        ac = ruler_codes()[1][0]
        word = lambda s: format(int(ac[s]) >> 16, "0%db" % (int(ac[s]) & 0xFF))
        return "0" + 3 * word(0xF0) + word(0xE8) + "11111111"

    def design(self):
        """(segment bit lengths, un-stuffed bytes) by the ruler's own arithmetic"""
        no_eob = self._no_eob_pattern()
        cost = np.array([2, 13, 13, 13, 5, 0, len(no_eob)])[self.kinds]
        start = np.concatenate(([0], np.cumsum(cost)[:-1]))
        T = int(cost.sum())
        bits = np.zeros(T + 8, np.uint8)
        bits[T:] = 1
        for k, pattern in ((1, "1011111111110"), (2, "1000000000000"), (3, "1001111111110"), (4, "11010"), (6, no_eob)):
            at = start[self.kinds == k]
            for i, ch in enumerate(pattern):
                if ch == "1":
                    bits[at + i] = 1
        raw = np.packbits(bits[:(T + 7) // 8 * 8]).tobytes()
        seg = np.add.reduceat(cost, np.arange(0, self.n, SEG_BLOCKS))
        return seg.astype(np.int64), raw

    def restart_design(self):
        """the same picture with every segment a restart interval: the DC predictor starts at 0, so an interval's first
        block, at level -511, costs 11 + 9 + 1 bits -- the code of size 9 is ten 1-bits and a 0, and an interval starts
        at a byte: EVERY interval begins with an 0xFF.  Returns the intervals' un-stuffed bytes (padded with 1-bits)."""
        firsts = np.arange(SEG_BLOCKS, self.n, SEG_BLOCKS)
        assert (self.kinds[firsts] == 0).all(), "an interval must start with a plain block"
        kinds = self.kinds.copy()
        kinds[firsts] = 5
        patterns = {1: "1011111111110", 2: "1000000000000", 3: "1001111111110", 4: "11010", 5: "111111111100000000000"}
        cost = np.array([2, 13, 13, 13, 5, 21])[kinds]
        out = []
        for lo in range(0, self.n, SEG_BLOCKS):
            k, c = kinds[lo:lo + SEG_BLOCKS], cost[lo:lo + SEG_BLOCKS]
            start = np.concatenate(([0], np.cumsum(c)[:-1]))
            T = int(c.sum())
            bits = np.ones((T + 7) // 8 * 8, np.uint8)
            bits[:T] = 0
            for kk, pattern in patterns.items():
                at = start[k == kk]
                for i, ch in enumerate(pattern):
                    if ch == "1":
                        bits[at + i] = 1
            out.append(np.packbits(bits).tobytes())
        return out

    def codes(self):
        return ruler_codes()

    def targets(self):
        """the bytes that are 0xFF by design"""
        if self.no_eob_at is not None:                     # (the byte across the two blocks: read off the written-out stream)
            return [i for i, b in enumerate(self.design()[1]) if b == 0xFF]
        out = []
        ups = list(self.pairs)
        if self.end_up:
            cost = np.array([2, 13, 13, 13, 5])[self.kinds]
            ups.append(int(cost[:-1].sum()))
        for p in ups:
            o = p + 2
            if o % 8 == 0:
                out.append(o // 8)
            elif o % 8 == 6:
                out.append((o + 2) // 8)
        return out

    def case(self, oracle=None):
        if self._case is None:
            levels = self.levels().astype(float)
            samples = np.floor(levels / 8.0)[:, None] + (np.arange(64)[None, :] < 8 * (levels % 8)[:, None])
            steps = {0: 1}
            if self.no_eob_at is not None:                 # (the basis function of zig-zag 63 is odd in x and y: the DC stays)
                samples[self.no_eob_at] += 255.5 * ec._BASIS[63]       # (what the oracle reads back as 255: pinned by the host test)
                steps[63] = 1
            field = ec._assemble(samples, self.bw)
            self._case = ec._paint(self.name, field, "gray", ec.quant_matrix(steps))
        return self._case


def aligned(byte):
    """start of the up-step block that makes `byte` an 0xFF"""
    return 8 * byte - 2


def _shift_pairs(n, first=20):
    """n up-steps that make no 0xFF (their 1-bits begin at bit 4 mod 8): each moves what follows by 22 bits"""
    out, p = [], first
    for _ in range(n):
        while (p + 2) % 8 != 4:
            p += 2
        out.append(p)
        p += 26
    return out


def _search(name, bw, bh, targets_of, wanted, form_of, max_shift=48, end_up=False):
    """the first count of shifting pairs in front under which the design reaches every event of `wanted`"""
    for n in range(max_shift):
        shift = _shift_pairs(n)
        first_free = (shift[-1] + 26) if shift else 18
        r = Ruler(name, bw, bh, shift, end_up)
        seg, raw = r.design()
        targets = targets_of(r, seg, first_free)
        if targets is None:
            continue
        try:
            r = Ruler(name, bw, bh, shift + [aligned(t) for t in targets], end_up)
        except AssertionError:
            continue
        seg, raw = r.design()
        ev = sm.events(seg, raw, 0, form_of(r))
        if all(ev[w] > 0 for w in wanted):
            return r
    raise AssertionError(f"no design of {name} reaches {wanted}")


MAIN_W, MAIN_H = 224, 220                                  # blocks: 1792 x 1760 pixels, 49 280 blocks, 201 segments


def _wide_form(r):
    return sm.uniform_form(1, r.nseg, 1 << 20)


@functools.lru_cache(maxsize=None)
def rulers():
    out = [Ruler("ruler-main", MAIN_W, MAIN_H, [aligned(t) for t in (8, 4095, 4100, 8192, 12287)])]
    # --- the lane straddle: a segment that crosses the first chunk boundary with wbeg mod 4 = 1, 2, 3, an FF in the
    # boundary's last word (chunk bytes 4092..4095) or first word (0..3)
    for m in (1, 2, 3):
        for side, byte in (("front", 4093), ("behind", 4097)):
            out.append(_search(f"ruler-straddle-{m}-{side}", 128, 132, lambda r, seg, free, byte=byte: [byte],
                               [f"K3 a lane's four words straddle a chunk boundary, wbeg mod 4 = {m}",
                                f"K3 lane straddles a chunk boundary with FF {'in front of' if side == 'front' else 'behind'} it"],
                               _wide_form))
    # --- an FF at each byte of an edge word: the word in which segment 20 ends
    for b in range(4):
        def at_edge(r, seg, free, b=b):
            end = int(np.cumsum(seg)[20])
            return [4 * (end >> 5) + b]
        out.append(_search(f"ruler-edge-byte{b}", 64, 96, at_edge, [f"K3 FF at byte {b} of an edge word"], _wide_form))
    # --- an FF in the frame's last word when that holds three bytes of the stream (the pair of steps is the picture's
    # last two blocks) and two (the last block steps up).  One byte -- the FF the stream's last byte -- needs a stream
    # that ends in 1-bits, and every block of a ruler ends with EOB = `0`: the band cases carry it.
    def at_end(r, seg, free):
        T = int(seg.sum()) + 22                            # (the target's own pair moves the end by 22 bits)
        return [(T - 24) // 8] if (T - 24) % 32 == 0 else None
    out.append(_search("ruler-last-word-3", 40, 37, at_end, ["K3 FF in the frame's last word, edge_valid = 3"], _wide_form))
    out.append(_search("ruler-last-word-2", 40, 37, lambda r, seg, free: [], ["K3 FF in the frame's last word, edge_valid = 2"],
                       _wide_form, end_up=True))
    # --- a last row of few blocks: the last segments hold a few bits each
    out.append(tiny_tail_ruler())
    return out


@functools.lru_cache(maxsize=None)
def restart_ruler():
    """restart mode: a marker whose two placeholder bytes lie at chunk bytes 4095 and 0, with the intervals' leading 0xFF
    bytes in front of it in its chunk"""
    wanted = "K6 placeholder straddles a chunk boundary with FF in front of it"
    for n in range(64):
        r = Ruler("ruler-restart", 128, 132, _shift_pairs(n))
        seg, raw = sm.restart_stream(r.restart_design())
        form = sm.uniform_form(1, r.nseg, 1 << 20, restart=True)
        if sm.events(seg, raw, 0, form)[wanted] > 0:
            return r
    raise AssertionError("no restart ruler")


def tiny_tail_ruler():
    """a picture ONE block wide has one block per MCU row; 246 * k + j blocks leave a last segment of j blocks = 2 j
    bits.  This one: two full segments and a last one of 1 block, 2 bits, in the word of the segment before."""
    return Ruler("ruler-tiny-tail", 1, 2 * SEG_BLOCKS + 1, [aligned(9), aligned(40)])


@functools.lru_cache(maxsize=None)
def tail_rulers():
    """last segments of 1..6 blocks (2..12 bits) behind segments whose end moves through the word"""
    return [Ruler(f"ruler-tail-{j}-{n}", 1, SEG_BLOCKS + j, _shift_pairs(n)) for j in (1, 2, 3, 6) for n in (0, 1, 2, 3, 5)]


# ---------------------------------------------------------------------------------------------- a stream that ends in 1-bits

@functools.lru_cache(maxsize=None)
def eob01_codes():
    """the ruler's DC table with an AC table whose EOB is `01` (symbol 0x01 takes `00`: the order of the symbols of one
    length is the table's to choose): a block that does not move costs `0` `01`, and the stream ends in a 1-bit"""
    dc = em.codes_from_lengths(RULER_DC, 12)[2]
    lengths = {s: 9 for s in ec.AC_SYMBOLS}
    lengths.update({0x00: 2, 0x01: 2})
    ac = em.codes_from_lengths(lengths, 256)[2]
    ac[0x00], ac[0x01] = (1 << 16) | 2, (0 << 16) | 2
    return np.stack([dc, dc]), np.stack([ac, ac])


class FlatRuler:
    """n flat blocks of level 0 in one row under eob01_codes(): 3 n bits, `001` each.  With 3 n = 1 (mod 8) the padded
    last byte is 1 + seven 1-bits = 0xFF: the stream's last byte is a stuffed FF."""

    def __init__(self, n, blocks_w=None):
        bw = n if blocks_w is None else blocks_w
        assert n % bw == 0
        self.name, self.n, self.bw, self.bh, self.nseg = f"ruler-flat-{n}", n, bw, n // bw, -(-n // SEG_BLOCKS)
        self.w, self.h = 8 * self.bw, 8 * self.bh
        self._case = None

    def codes(self):
        return eob01_codes()

    def targets(self):
        raw = self.design()[1]
        return [i for i, b in enumerate(raw) if b == 0xFF]

    def design(self):
        bits = np.tile(np.array([0, 0, 1], np.uint8), self.n)
        seg = np.array([3 * min(SEG_BLOCKS, self.n - lo) for lo in range(0, self.n, SEG_BLOCKS)], np.int64)
        return seg, sm.raw_stream([bits])[0]

    def case(self, oracle=None):
        if self._case is None:
            self._case = ec._paint(self.name, np.zeros((self.h, self.w)), "gray", ec.quant_matrix({0: 1}))
        return self._case


@functools.lru_cache(maxsize=None)
def flat_rulers():
    """padded last byte FF with two bytes and with one byte of the stream in the frame's last word (3, 11 blocks), and
    not FF (2, 8 blocks: T mod 8 = 6 and 0)"""
    return [FlatRuler(n) for n in (3, 11, 2, 8)]


# ---------------------------------------------------------------------------------------------- dense prefix

class DenseRuler:
    """`nprefix` blocks of pixel noise in front of a ruler: its AC coefficients at zig-zag 1..npos are coded (step 16), so
    that the segments of the prefix are hundreds of words long.  Where the ruler part starts and at which DC level is
    taken from the model (the oracle's coefficients of the prefix alone), then the ruler's arithmetic goes on from
    there: `targets` are bytes counted from where the ruler part starts."""

    def __init__(self, name, blocks_w, blocks_h, nprefix, npos, targets, seed):
        self.name, self.bw, self.bh, self.nprefix, self.npos = name, blocks_w, blocks_h, nprefix, npos
        self.n = blocks_w * blocks_h
        self.w, self.h = 8 * blocks_w, 8 * blocks_h
        self.nseg = -(-self.n // SEG_BLOCKS)
        self._targets, self.seed = list(targets), seed
        self._case = None

    def quant(self):
        steps = {p: 16 for p in range(1, self.npos + 1)}
        steps[0] = 1
        return ec.quant_matrix(steps)

    def case(self, oracle):
        if self._case is not None:
            return self._case
        dc, ac = ruler_codes()
        rs = np.random.RandomState(self.seed)
        noise = rs.randint(-120, 121, (self.nprefix, 64)).astype(float)
        # the prefix alone, through the oracle and the model: its bits and its last DC level
        pre = ec._paint(self.name + "-prefix", ec._assemble(noise, self.nprefix), "gray", self.quant())
        zz = oracle.scan_coeffs(pre.rgb, pre.quant, yuv_mode=em.YUV_400)
        _, tr = em.encode_scan(zz, em.YUV_400, dc, ac)
        pos, level = tr.total_bits, int(zz[-1][0])
        lens = em.lengths_of(dc[0])

        def cost(a, b):
            n = abs(b - a).bit_length()
            return lens[n] + n + 1
        # to level -511 at an even bit: directly, or over a neighbour
        for via in ((), (-512,), (-510,), (-512, -510), (-509,)):
            path = [level, *via, -511]
            c = sum(cost(path[i], path[i + 1]) for i in range(len(path) - 1))
            if (pos + c) % 2 == 0:
                break
        else:
            raise AssertionError("no connection of even length")
        levels = list(path[1:])
        pos += c
        self.ruler_from = pos
        self.pairs = []
        for t in sorted(self._targets):                    # (bytes behind the ruler's first whole byte)
            p = aligned((self.ruler_from + 7) // 8 + t)
            assert (p - pos) % 2 == 0
            levels += [-511] * ((p - pos) // 2) + [512, -511]
            self.pairs.append(p)
            pos = p + 26
        assert self.nprefix + len(levels) <= self.n
        levels += [-511] * (self.n - self.nprefix - len(levels))
        lv = np.array(levels, float)
        samples = np.floor(lv / 8.0)[:, None] + (np.arange(64)[None, :] < 8 * (lv % 8)[:, None])
        field = ec._assemble(np.concatenate((noise, samples)), self.bw)
        self._case = ec._paint(self.name, field, "gray", self.quant())
        return self._case

    def targets(self):
        return [(p + 2) // 8 for p in self.pairs]

    def codes(self):
        return ruler_codes()


@functools.lru_cache(maxsize=None)
def dense_rulers():
    """a segment above 768 words, one above 1024, and one longer than its slot at a capacity that still fits"""
    return [DenseRuler("dense-ruler-768", 41, 18, 246, 7, (4, 9, 40, 100), 11),
            DenseRuler("dense-ruler-1024", 41, 18, 246, 16, (5, 10, 63), 12),
            DenseRuler("dense-ruler-pool", 41, 18, 2 * 246, 24, (6, 11, 17), 13)]


# ---------------------------------------------------------------------------------------------- picture (c)

NOISE_W, NOISE_H = 512, 480


@functools.lru_cache(maxsize=None)
def saturated_noise():
    """one gray frame of byte noise, every quantizer step 1: 66 chunks of un-stuffed stream or more under the standard
    tables (asserted on the model by the host test)"""
    from oracle import synth
    g = synth.g_noise(NOISE_W, NOISE_H, 660066)[:, :, :1]
    return ec.Case("saturated-noise", np.repeat(g, 3, 2), em.YUV_400, np.ones((2, 64), np.uint8))


# ---------------------------------------------------------------------------------------------- routes

FUSED1_STRIDE = 1 << 20                                    # 257 chunks of scratch: K4 inside K5, K2 inside K3 (form 1)
FUSED2_STRIDE = 12 << 20                                   # 3073 chunks: one frame above 2048 takes form 2


@functools.lru_cache(maxsize=None)
def big_rulers():
    """Pictures of 158 segments or more: below that a frame's scratch, capped at its segments' worst case, stays under
    2 049 chunks whatever out_stride says, and the uniform entry never takes fused form 2.  Together with the main ruler
    they carry every place of K3's wide form and K5 at that size (the shift counts were searched once on the design's
    arithmetic and are written out; tests/test_stitch_model_host.py asserts the events they reach)."""
    straddle = []
    at = 20
    for n, boundary in ((2, 4096), (1, 8192), (2, 12288)):  # shifting steps, then an FF on either side of a chunk boundary
        straddle += _shift_pairs(n, at) + [aligned(boundary - 3), aligned(boundary + 1)]
        at = aligned(boundary + 1) + 26
    straddle += _shift_pairs(3, at)
    total = 2 * MAIN_W * MAIN_H + 14 + 22 * (len(straddle) + 1)
    straddle.append(total - 26)                            # the last two blocks: FF at byte 0 of the frame's last word, 3 valid
    edges = [11326, 25126, 39918, 54710]                   # FF at byte 0..3 of the words in which segments 22, 50, 80, 110 end
    edges += _shift_pairs(8, edges[-1] + 26)               # ... and the last block's step up makes an FF with 2 valid bytes
    return [Ruler("ruler-big-straddle", MAIN_W, MAIN_H, straddle),
            Ruler("ruler-big-edges", 246, 158, edges, end_up=True),
            # a last segment of ONE block (2 bits) behind 158 full ones: edge_easy false, edge_valid 3, 2, 1 in the word
            # of the segment before
            Ruler("ruler-big-tail-0", 47, 827, _shift_pairs(0)),
            Ruler("ruler-big-tail-1", 47, 827, _shift_pairs(1)),
            Ruler("ruler-big-tail-2", 47, 827, _shift_pairs(2)),
            # the last block of segment 9 ends in eight 1-bits without EOB, segment 10 starts with `10`: seven and one
            # make byte 624 an 0xFF of two segments' bits
            Ruler("ruler-big-two-segments", 246, 158, _shift_pairs(1), no_eob_at=10 * SEG_BLOCKS - 1),
            FlatRuler(38955, 105),                         # 3 n = 1 (mod 32): the padded last byte FF, alone in the last word
            DenseRuler("dense-ruler-big", 246, 158, 2 * SEG_BLOCKS, 16, (5, 10, 63), 14)]


def pictures():
    """every ruler picture, in the order the routes take them"""
    return rulers() + tail_rulers() + dense_rulers() + flat_rulers() + big_rulers()


def tight(nbytes):
    return (nbytes + 15) & ~15


def uniform_routes(pic, jpeg_len, header_len):
    """route -> (out_stride, form) of the uniform entries for one picture whose whole stream has jpeg_len bytes (the
    entry refuses an out_stride below header + 2 + 64)"""
    t = tight(max(jpeg_len, header_len + 2 + 64))
    routes = {"fused 1, tight": (t, sm.uniform_form(1, pic.nseg, t)),
            "fused 1": (FUSED1_STRIDE, sm.uniform_form(1, pic.nseg, FUSED1_STRIDE)),
            "fused 2": (FUSED2_STRIDE, sm.uniform_form(1, pic.nseg, FUSED2_STRIDE)),
            "packed, 4 frames": (FUSED1_STRIDE, sm.uniform_form(4, pic.nseg, FUSED1_STRIDE, packed=True)),
            "per-frame tables, 3 frames": (FUSED1_STRIDE, sm.uniform_form(3, pic.nseg, FUSED1_STRIDE))}
    # (the scratch of a frame is capped at its segments' worst case: below 158 segments no out_stride gives 2049 chunks)
    if routes["fused 2"][1]["fused_k4"] != 2:
        del routes["fused 2"]
    return routes
