"""Pictures designed in the coefficient domain, and families of Huffman tables.  TEST INFRASTRUCTURE.

A picture is built block by block: a plan of dequantized DCT coefficients (zig-zag order) goes through a float
IDCT, is clipped and rounded to pixels, and is coded with a quant matrix of its own -- 1, or a chosen step, at the
planned positions, 255 everywhere else, so that the harmonics of a clipped cosine and the rounding noise quantize to
zero.  Luma plans make gray pictures (R = G = B, 4:0:0), chroma plans 4:4:4 pictures mixed between yellow and blue
(Cb) or red and cyan (Cr) by the plan.  What a picture really holds is what oracle.scan_coeffs reads back, never
what was planned: the coverage conditions of test_entropy_model_host.py are asserted on the model's trace.
"""
import functools

import numpy as np

import entropy_model as em

YUV_420, YUV_444, YUV_400 = em.YUV_420, em.YUV_444, em.YUV_400
# zig-zag position -> natural index (row * 8 + column)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
          53, 60, 61, 54, 47, 55, 62, 63)
LEVELS = (1, 2, 3, 4, 6, 7, 8, 12, 15, 16, 24, 31, 32, 48, 63, 64, 96, 127, 128, 192, 255, 256, 384, 511, 512, 768, 1023)
GAINS = (1.0, 1.25, 1.6, 2.2, 3.5)


def _basis():
    x = np.arange(8)
    c = np.cos((2 * x[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)      # [x][u]
    c[:, 0] *= np.sqrt(0.5)
    b = np.zeros((64, 8, 8))
    for p, nat in enumerate(ZIGZAG):
        v, u = divmod(nat, 8)
        b[p] = 0.25 * np.outer(c[:, v], c[:, u])
    return b.reshape(64, 64)


_BASIS = _basis()                                          # zig-zag position -> the 64 samples of its basis function


class Case:
    """one picture: its pixels, its sampling, its quant matrices [2][64] (natural order)"""

    def __init__(self, name, rgb, yuv_mode, quant):
        self.name, self.rgb, self.yuv_mode = name, np.ascontiguousarray(rgb, np.uint8), yuv_mode
        self.quant = np.ascontiguousarray(quant, np.uint8).reshape(2, 64)
        self.h, self.w = self.rgb.shape[:2]
        self._zz = self._symbols = None

    def coeffs(self, oracle):
        if self._zz is None:
            self._zz = oracle.scan_coeffs(self.rgb, self.quant, yuv_mode=self.yuv_mode)
        return self._zz

    def symbols(self, oracle):
        """the scan's items, walked once; every table family codes them again (entropy_model.encode_symbols)"""
        if self._symbols is None:
            self._symbols = em.Symbols(self.coeffs(oracle), self.yuv_mode)
        return self._symbols

    def __repr__(self):
        return self.name


def quant_matrix(steps, rest=255):
    """{zig-zag position: step} -> one matrix in natural order"""
    q = np.full(64, rest, np.uint8)
    for p, s in steps.items():
        q[ZIGZAG[p]] = s
    return q


def _assemble(samples, blocks_w):
    """[n][64] float samples around 0 -> [rows * 8][blocks_w * 8] float, the last row of blocks padded with zeros"""
    n = samples.shape[0]
    rows = -(-n // blocks_w)
    full = np.zeros((rows * blocks_w, 64))
    full[:n] = samples
    return full.reshape(rows, blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, blocks_w * 8)


_PAIRS = {"yb": ((255, 255, 0), (0, 0, 255)),              # Cb: 1 .. 255
          "rc": ((0, 255, 255), (255, 0, 0))}              # Cr: 1 .. 255


def _paint(name, field, colour, mine, other=None):
    """A field of samples around 0 as a picture: gray (4:0:0, the field is its luma) or "yb" / "rc" (4:4:4, the field is
    about its Cb / Cr).  mine: the matrix of the field's table; other: the other table's (default: 255 everywhere)."""
    theirs = np.full(64, 255, np.uint8) if other is None else other
    if colour == "gray":
        g = np.clip(np.rint(128.0 + field), 0, 255).astype(np.uint8)
        return Case(name, np.repeat(g[:, :, None], 3, 2), YUV_400, [mine, theirs])
    lo, hi = (np.array(c, float) for c in _PAIRS[colour])
    t = (np.clip(field / 127.0, -1.0, 1.0) + 1.0) / 2.0
    rgb = np.rint(lo[None, None, :] + t[:, :, None] * (hi - lo)[None, None, :])
    return Case(name, rgb.astype(np.uint8), YUV_444, [theirs, mine])


def picture(name, plans, blocks_w, quant_steps, colour="gray", rest=255, other=None):
    """plans: [n][64] dequantized coefficients, zig-zag order, through the float IDCT.  quant_steps: the planned
    positions' steps of the plan's table (the rest: `rest`)."""
    field = _assemble(np.asarray(plans, float) @ _BASIS, blocks_w)
    return _paint(name, field, colour, quant_matrix(quant_steps, rest), other)


# ---------------------------------------------------------------------------------------------- pictures

def _atlas_plans(pos, levels, gains, early=None):
    plans = []
    for g in gains:
        for lv in levels:
            for sign in (1, -1):
                p = np.zeros(64)
                p[pos] = sign * lv * g
                if early is not None:
                    p[early] = 40.0 * sign
                plans.append(p)
    return np.array(plans)


@functools.lru_cache(maxsize=None)
def atlas(colour):
    """One picture per run 0..15 and quarter 0..3: the planned coefficient is the first symbol of the block (quarter 0,
    zig-zag position run + 1) or, behind one earlier coefficient at the last position of the quarter before, the first
    of quarter 1, 2 or 3 -- inside a merged part where the block is lean (quarters 1 and 3)."""
    out = []
    for run in range(16):
        out.append(picture(f"atlas-{colour}-q0-run{run}", _atlas_plans(run + 1, LEVELS, GAINS), 27, {run + 1: 1}, colour))
        for q in (1, 2, 3):
            early, pos = 16 * q - 1, 16 * q + run
            out.append(picture(f"atlas-{colour}-q{q}-run{run}", _atlas_plans(pos, LEVELS, GAINS[::2], early), 27,
                               {pos: 1, early: 16}, colour))
    return out


def _dc_walk():
    """DC levels -1024 .. 1016 whose differences take every size 0..11 with either sign, at both ends of a size"""
    seq = []
    for m in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2040):
        lo = -(m // 2) - (4 if m == 2040 else 0)
        seq += [lo, lo + m, lo, lo + m]
    return seq


@functools.lru_cache(maxsize=None)
def dc_pictures():
    """600 blocks (25 x 24): three segments of 4:0:0, eight of 4:4:4; the walk repeats with a shifting phase, so that
    the differences cross MCU rows and segment boundaries (the predictor then comes from the halo MCU)."""
    walk = _dc_walk()
    levels = np.array([walk[(i + i // len(walk)) % len(walk)] for i in range(600)], float)
    # a DC level d is a flat block of 128 + floor(d / 8) with 8 * (d mod 8) of its samples one higher: the AC this makes
    # disappears under the step of 255
    samples = np.floor(levels / 8.0)[:, None] + (np.arange(64)[None, :] < 8 * (levels % 8)[:, None])
    field = _assemble(samples, 25)
    dc_only = quant_matrix({0: 1})
    # (the luma of a two-colour picture moves with its chroma: its DC step is 1 as well)
    return [_paint(f"dc-{colour}", field, colour, dc_only, None if colour == "gray" else dc_only)
            for colour in ("gray", "yb", "rc")]


@functools.lru_cache(maxsize=None)
def zrl_pictures():
    """Blocks whose only AC coefficients lie at zig-zag positions p0 < p (p0 = 0: the DC alone in front) with a run of
    16 .. 62 between them: k = 1, 2 and 3 ZRL codes in front of a symbol in quarter 1, 2 or 3, behind DC differences of
    every length, so that the chains start at every bit offset.  All AC steps 8, levels 1..7: nothing clips."""
    rs = np.random.RandomState(20240611)
    plans = []
    for k in (1, 2, 3):
        for _ in range(336):
            run = 16 * k + rs.randint(0, 15 if k == 3 else 16)
            p0 = rs.randint(0, 63 - run)
            p = p0 + run + 1
            pl = np.zeros(64)
            pl[0] = rs.randint(-600, 601)
            if p0:
                pl[p0] = 8 * rs.randint(1, 8) * rs.choice((-1, 1))
            pl[p] = 8 * rs.randint(1, 8) * rs.choice((-1, 1))
            plans.append(pl)
    plans = np.array(plans)[rs.permutation(len(plans))]
    steps = {p: 8 for p in range(1, 64)}
    steps[0] = 1
    out = []
    for colour in ("gray", "yb", "rc"):
        other = quant_matrix(steps) if colour != "gray" else None
        out.append(picture(f"zrl-{colour}", plans, 28, steps, colour, other=other))
    return out


@functools.lru_cache(maxsize=None)
def bound_pictures():
    """Blocks whose largest AC level has n bits, n = 0..10 in turn, twice per segment and more: the large level at
    zig-zag position 1, or alone in quarter 3 (position 50) with levels of one bit elsewhere."""
    plans = []
    rs = np.random.RandomState(77)
    for i in range(492):
        n = i % 11
        pl = np.zeros(64)
        pl[0] = rs.randint(-200, 201)
        if n:
            lv = rs.randint(1 << (n - 1), 1 << n) * rs.choice((-1, 1))
            high = (i // 11) % 3 == 2 and n <= 8
            pl[50 if high else 1] = lv * (1.0 if n < 9 else 1.5)
            if high or (i // 11) % 3 == 1:
                for p in (5, 20, 37):
                    pl[p] = 8 * rs.choice((-1, 1))
        plans.append(pl)
    steps = {p: 8 for p in range(2, 64)}
    steps.update({0: 4, 1: 1, 50: 1})
    return [picture(f"bound-{colour}", np.array(plans), 41, steps, colour)
            for colour in ("gray", "yb")]


@functools.lru_cache(maxsize=None)
def dense_pictures():
    """quantized noise, 58 to 63 of the 63 AC coefficients of every block non-zero (all steps 1): one, two and three segments of
    246 blocks of 4:0:0, 82 MCUs of 4:4:4 and 41 MCUs of 4:2:0"""
    from oracle import synth
    out = []
    ones = np.ones((2, 64), np.uint8)
    for mode, name, px, seg in ((YUV_400, "400", 8, 246), (YUV_444, "444", 8, 82), (YUV_420, "420", 16, 41)):
        for nseg in (1, 2, 3):
            rgb = synth.g_noise(px * seg, px * nseg, 1000 + 10 * mode + nseg)
            if mode == YUV_400:
                rgb = np.repeat(rgb[:, :, :1], 3, 2)
            out.append(Case(f"dense-{name}-{nseg}seg", rgb, mode, ones))
    return out


FIB_QUALITY = 50.0
FIB_SYMBOLS = 22


@functools.lru_cache(maxsize=None)
def fibonacci_picture(oracle_quant_luma):
    """A gray picture for the product's own optimiser: one planned AC symbol per block, (run, size) with size 1..3,
    the block counts of the symbols the Fibonacci numbers -- the unrestricted Huffman code of such counts is a comb
    as deep as there are symbols, and the optimiser has to cut it to 16 bits.  oracle_quant_luma: the 64 luma steps
    (natural order) of FIB_QUALITY, as a tuple."""
    q = np.array(oracle_quant_luma, float)
    fib = [1, 1]
    while len(fib) < FIB_SYMBOLS:
        fib.append(fib[-1] + fib[-2])
    symbols = [(run, size) for size in (1, 2, 3) for run in range(16)][:FIB_SYMBOLS]
    plans = []
    rs = np.random.RandomState(5)
    for (run, size), count in zip(symbols[::-1], fib):      # the rarest symbol: the last of the list
        for _ in range(count):
            lv = rs.randint(1 << (size - 1), 1 << size) * rs.choice((-1, 1))
            pl = np.zeros(64)
            pl[run + 1] = lv * q[ZIGZAG[run + 1]]
            plans.append(pl)
    plans = np.array(plans)[rs.permutation(len(plans))]
    side = int(np.ceil(np.sqrt(len(plans))))
    field = _assemble(plans @ _BASIS, side)
    g = np.clip(np.rint(128.0 + field), 0, 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, 2)


def huffman_depth(freq):
    """depth of the unrestricted Huffman code of the non-zero counts in freq, with the reserved all-ones symbol"""
    import heapq
    heap = [(int(f), 0) for f in freq if f] + [(0, 0)]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def directed_pictures():
    """every picture the table families are run over"""
    return (atlas("gray") + atlas("yb") + dc_pictures() + zrl_pictures() + bound_pictures() + dense_pictures())


# ---------------------------------------------------------------------------------------------- table families

AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


def _fill(lengths, rest):
    out = {s: rest for s in AC_SYMBOLS}
    out.update(lengths)
    return out


def ac_family(name):
    """{symbol: length} of one AC table of the family `name`"""
    kind, _, arg = name.partition(":")
    n = int(arg) if arg else 0
    if kind == "safe":
        # len(0, n') + n' == 16 exactly up to n, and the longest code on (0, n + 1)
        lengths = {s: 16 - s for s in range(1, n + 1)}
        if n < 10:
            lengths[n + 1] = 16
        return _fill(lengths, 10)
    if kind == "zrl":
        # shorter codes in front of the ZRL's and codes of its own length beside it: a pattern with bits set at both ends
        if n == 1:
            return _fill({0xF0: 1}, 9)
        if n == 2:
            return _fill({0x00: 2, 0xF0: 2}, 9)
        if n == 3:
            return _fill({0x00: 2, 0x01: 2, 0x02: 3, 0xF0: 3}, 10)
        return _fill({0x00: 2, 0x01: 2, 0x02: 3, 0x03: n, 0x04: n, 0xF0: n}, 10)
    if kind == "eob":
        if n == 1:
            return _fill({0x00: 1}, 9)
        return _fill({0x01: 2, 0x02: 2, 0x03: 3, 0x00: n}, 10)
    if kind == "long":
        return _fill({}, 16)
    raise KeyError(name)


AC_FAMILIES = ([f"safe:{n}" for n in range(11)] + [f"zrl:{n}" for n in range(1, 17)] + [f"eob:{n}" for n in (1, 8, 16)]
               + ["long"])
APPLY = ("luma", "chroma", "both")
DC_LONG = {0: 2, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 4, 7: 5, 8: 6, 9: 12, 10: 14, 11: 16}


def family_codes(oracle, name, apply="both"):
    """(dc_codes[2][12], ac_codes[2][256]) of a family: the family's AC table for luma, chroma or both, the other table
    standard; DC standard, but all of 16 bits under `long` and DC_LONG under `dc_long`."""
    dc, ac = oracle.default_codes()
    dc, ac = dc.copy(), ac.copy()
    which = {"luma": (0,), "chroma": (1,), "both": (0, 1)}[apply]
    if name == "std":
        return dc, ac
    if name == "dc_long":
        for t in which:
            dc[t] = em.codes_from_lengths(DC_LONG, 12)[2]
        return dc, ac
    for t in which:
        ac[t] = em.codes_from_lengths(ac_family(name), 256)[2]
        if name == "long":
            dc[t] = em.codes_from_lengths({s: 16 for s in range(12)}, 12)[2]
    return dc, ac
