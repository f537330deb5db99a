"""A plain stitch -- bit strings to one byte-stuffed stream -- and a record of where the stitch kernels decide.
TEST INFRASTRUCTURE.

`stitch()` is the reference: concatenate the bits, pad the last byte with 1-bits, FF -> FF 00, header in front, EOI
behind.  Plain Python / numpy; nothing of it is shared with the kernels.

`events()` names the decision points of K2..K6 (sjpeg_amd/csrc/stitch_kernels.h) that a stream reaches.  It is worked out
from the STREAM alone -- the segments' bit lengths and the un-stuffed bytes -- never from what the code under test did.
What the host decides (the `form`: slot words, chunk scratch, fused kernels, waves per segment, workgroups per frame) is
RESTATED here from DESIGN.md section 3 and the comments of seg_plan() / the launch code, never imported.  The library
exposes no way to read the form of a launch back: which form a case is EXPECTED to take is this file's arithmetic
(`uniform_form`, `ragged_form`, `band_form`), and the tests rest on it being the library's.
"""
from collections import Counter

import numpy as np

import entropy_model as em

CHUNK = 4096                       # bytes of un-stuffed stream per K5 workgroup step
CHUNK_WORDS = 1024
GROUP = 16                         # bytes per K5 thread
THREADS = 256
WAVE_WORDS = 768                   # words of a segment one K3 wave has requested before its offsets arrive
FUSED_CHUNKS, FUSED_SEGS = 2048, 2048
FUSED_CHUNKS_BIG, FUSED_SEGS_BIG = 1 << 17, 16384
WORST_SLOT = ((246 * em.MAX_BLOCK_BITS + 31) // 32 + 2 + 3) & ~3


# ---------------------------------------------------------------------------------------------- the reference

def bits_of(words, nbits):
    """MSB-first uint32 words -> array of nbits 0/1"""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32).astype(">u4"))
    return np.unpackbits(w.view(np.uint8))[:nbits]


def words_of(bits, stride=None):
    """0/1 array -> MSB-first words as int32 (what the band entry takes), zero bits behind the last"""
    bits = np.asarray(bits, np.uint8)
    n = (len(bits) + 31) // 32
    by = np.zeros((stride if stride is not None else max(n, 1)) * 4, np.uint8)
    packed = np.packbits(bits)
    by[:len(packed)] = packed
    return by.view(">u4").astype(np.uint32).view(np.int32)


def raw_stream(bit_strings):
    """(un-stuffed bytes with the last byte padded with 1-bits, total bits)"""
    bits = np.concatenate([np.asarray(b, np.uint8) for b in bit_strings] + [np.zeros(0, np.uint8)])
    total = len(bits)
    if total & 7:
        bits = np.concatenate([bits, np.ones(8 - (total & 7), np.uint8)])
    return np.packbits(bits).tobytes(), total


def stuff(raw):
    out = bytearray()
    for b in bytes(raw):                                   # (byte by byte on purpose: the plainest form there is)
        out.append(b)
        if b == 0xFF:
            out.append(0)
    return bytes(out)


def stitch(bit_strings, header=b"", append_eoi=True):
    raw, _ = raw_stream(bit_strings)
    return bytes(header) + stuff(raw) + (b"\xff\xd9" if append_eoi else b"")


# ---------------------------------------------------------------------------------------------- restart form

def encode_restart(zz, yuv_mode, dc_codes, ac_codes):
    """The scan with every segment a restart interval: predictors reset, each interval padded with 1-bits to a byte,
    RSTn between intervals.  Returns (stuffed bytes with markers, the intervals' un-stuffed bytes)."""
    zz = np.asarray(zz)
    per = em.SEGMENT_MCUS[yuv_mode] * len(em.MCU_COMPONENTS[yuv_mode])
    out, raws = bytearray(), []
    nseg = -(-zz.shape[0] // per)
    for s in range(nseg):
        body, _ = em.encode_scan(zz[s * per:(s + 1) * per], yuv_mode, dc_codes, ac_codes)
        raws.append(body.replace(b"\xff\x00", b"\xff"))
        out += body
        if s != nseg - 1:
            out += bytes((0xFF, 0xD0 + (s & 7)))
    return bytes(out), raws


def restart_stream(raws):
    """what the stitch kernels see in restart mode: every interval but the last with 16 zero bits behind it
    (segment bit lengths, un-stuffed bytes)"""
    seg_bits = [8 * len(r) + (16 if i != len(raws) - 1 else 0) for i, r in enumerate(raws)]
    return np.array(seg_bits, np.int64), b"\x00\x00".join(raws)


# ---------------------------------------------------------------------------------------------- the host's plan

def _ubuf_words(budget_words):
    return (budget_words + CHUNK_WORDS + 3) & ~3


def _frame_plan(capacity, nseg):
    budget = min(capacity // 4 + 16, nseg * WORST_SLOT)
    ubuf = _ubuf_words(budget)
    return em.slot_words(capacity, nseg), ubuf, (ubuf + CHUNK_WORDS - 1) // CHUNK_WORDS


def uniform_form(nframes, nseg, capacity, packed=False, restart=False, out_align=0):
    """sjpeg_hip_encode_scan and its kin: `capacity` is out_stride"""
    slot, ubuf, max_chunks = _frame_plan(capacity, nseg)
    few = nframes * nseg <= 8192
    subs = (slot + WAVE_WORDS - 1) // WAVE_WORDS if few and slot % 4 == 0 and slot >= 776 else 1
    fuse_ok = few and not packed and not restart
    fused4 = 0 if not fuse_ok else 1 if max_chunks <= FUSED_CHUNKS else 2 if nframes == 1 and max_chunks <= FUSED_CHUNKS_BIG else 0
    fused2 = 0 if not fused4 else 1 if fused4 == 1 and nseg <= FUSED_SEGS else 2 if nseg <= FUSED_SEGS_BIG and nframes == 1 else 0
    return dict(slot_words=slot, ubuf_words=ubuf, max_chunks=max_chunks, subs=subs, wide_subs=subs > 1,
                wide=slot % 4 == 0 and slot >= 776, fused_k2=fused2, fused_k4=fused4, ragged=False, pool=True,
                gx=min(max(4096 // nframes, 64), max_chunks), out_align=out_align, restart=restart, packed=packed)


def ragged_form(capacities, nsegs, k, out_align=0):
    """frame k of one ragged launch: the slot is the launch's largest, one wave per segment, no fused form"""
    plans = [_frame_plan(c, n) for c, n in zip(capacities, nsegs)]
    slot = max(p[0] for p in plans)
    return dict(slot_words=slot, ubuf_words=plans[k][1], max_chunks=plans[k][2], subs=1, wide_subs=False,
                wide=slot % 4 == 0 and slot >= 776, fused_k2=0, fused_k4=0, ragged=True, pool=True,
                gx=min(max(4096 // len(plans), 64), plans[k][2]), out_align=out_align, restart=False, packed=False)


def band_form(nbands, stride, out_align=0):
    """sjpeg_hip_stitch_bands: bands as segments, the narrow form of K3, no pool"""
    ubuf = _ubuf_words(nbands * stride)
    max_chunks = (ubuf + CHUNK_WORDS - 1) // CHUNK_WORDS
    return dict(slot_words=stride, ubuf_words=ubuf, max_chunks=max_chunks, subs=(stride + WAVE_WORDS - 1) // WAVE_WORDS,
                wide_subs=False, wide=False, fused_k2=0, fused_k4=0, ragged=False, pool=False, bands=True,
                gx=min(4096, max_chunks), out_align=out_align, restart=False, packed=False)


# ---------------------------------------------------------------------------------------------- events

def _k5_events(ev, raw, total_bits, header_size, form):
    U = len(raw)
    if total_bits & 7:
        ev[f"K5 T mod 8 = {total_bits & 7}: the padded last byte is {'FF' if raw[-1] == 0xFF else 'not FF'}"] += 1
    else:
        ev[f"K5 T mod 8 = 0: the last byte is {'FF' if raw[-1] == 0xFF else 'not FF'}"] += 1
    a = np.frombuffer(raw, np.uint8)
    ff = a == 0xFF
    nchunks = -(-U // CHUNK)
    ng = -(-U // GROUP)
    # the stream as K3 leaves it in memory: the last word's bytes behind the stream's end are 1-bits
    mem = np.full(ng * GROUP + 4, False)
    mem[:U] = ff
    mem[U:((U + 3) & ~3)] = True
    g_ff = mem[:ng * GROUP].reshape(ng, GROUP).copy()
    valid = np.minimum(U - GROUP * np.arange(ng), GROUP)
    g_ff[np.arange(GROUP)[None, :] >= valid[:, None]] = False
    nff = g_ff.sum(1)
    # the word behind a thread's bytes is read only while it holds a byte of the stream
    has_behind = GROUP * (np.arange(ng) + 1) < U
    beh = np.zeros((ng, 4), bool)
    idx = GROUP * (np.arange(ng) + 1)
    for b in range(4):
        beh[:, b] = mem[np.minimum(idx + b, len(mem) - 1)] & has_behind
    behind_plain = ~beh[:, :3].any(1)
    fast = (valid == GROUP) & (nff == 0) & behind_plain
    nbeh = beh.sum(1)
    state = np.where(nbeh == 0, -1, np.where(nbeh == 1, beh.argmax(1), -2))      # -1 plain, 0..3 the only one, -2 several
    sname = {-1: "plain", 0: "ff@0", 1: "ff@1", 2: "ff@2", 3: "ff@3"}
    full = valid == GROUP
    for g in np.nonzero(full & (nff == 1) & (state > -2))[0]:
        ev[f"K5 group: ff@{int(g_ff[g].argmax())} behind {sname[int(state[g])]}"] += 1
    for g in np.nonzero(full & (nff == 0) & (state >= 0))[0]:
        ev[f"K5 group: plain behind {sname[int(state[g])]} ({'fast' if fast[g] else 'slow'})"] += 1
    ev["K5 group: fast"] += int(fast.sum())
    ev["K5 group: slow"] += int((~fast).sum())
    same_chunk = (np.arange(ng - 1) + 1) % THREADS != 0
    ev["K5 slow thread in front of a fast one"] += int((~fast[:-1] & fast[1:] & same_chunk).sum())
    ev["K5 fast thread in front of a slow one"] += int((fast[:-1] & ~fast[1:] & same_chunk).sum())
    last_thread = np.arange(ng) % THREADS == THREADS - 1
    ev["K5 last thread of a chunk slow by the next chunk's first bytes"] += int((last_thread & full & (nff == 0) & ~behind_plain).sum())
    # runs of FF bytes, against the boundaries of groups and chunks
    d = np.diff(np.concatenate(([0], ff.astype(np.int8), [0])))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    for s, e in zip(starts.tolist(), ends.tolist()):         # run = bytes s .. e - 1
        n = e - s
        if n > 5 and n < CHUNK:
            continue
        for unit, name in ((GROUP, "group"), (CHUNK, "chunk")):
            first_boundary = (s // unit + 1) * unit
            if n >= 2 and s < first_boundary < e:
                ev[f"K5 run of {min(n, CHUNK)} FF across a {name} boundary"] += 1
            if n == 1 and (s % unit == unit - 1 or (s % unit == 0 and s > 0)):
                ev[f"K5 run of 1 FF at a {name} boundary"] += 1
    for c in range(nchunks):
        lo, hi = c * CHUNK, min((c + 1) * CHUNK, U)
        if hi - lo == CHUNK and ff[hi - 1]:
            ev["K5 FF is the last byte of a full chunk"] += 1
        if c > 0 and ff[lo]:
            ev["K5 FF is the first byte of a chunk behind the first"] += 1
        if hi - lo == CHUNK and ff[lo:hi].all():
            ev["K5 chunk of 4096 FF"] += 1
    if U % GROUP:
        ev[f"K5 last thread has {U % GROUP} bytes"] += 1
    if U % CHUNK in (0, 1, CHUNK - 1) and U >= CHUNK - 1:
        ev["K5 U = 4096 k" + {0: "", 1: " + 1", CHUNK - 1: " - 1"}[U % CHUNK]] += 1
    if U <= 17:
        ev[f"K5 U = {U}"] += 1
    # where a chunk lands, and how it is copied out
    counts = np.add.reduceat(ff.astype(np.int64), np.arange(0, U, CHUNK)) if U else np.zeros(0, np.int64)
    front = np.concatenate(([0], np.cumsum(counts)[:-1]))
    for c in range(nchunks):
        mis = (form["out_align"] + header_size + c * CHUNK + int(front[c])) & 15
        ev[f"K5 mis = {mis} ({'first chunk' if c == 0 else 'later chunk'})"] += 1
        nbytes = min(CHUNK, U - c * CHUNK) + int(counts[c])
        if ((mis + 15) & ~15) > ((mis + nbytes) & ~15):
            ev["K5 copy-out byte by byte (no aligned 16 inside)"] += 1
    ev["K5 chunk offset from " + {0: "co[] (K4)", 1: "fused_off[] (LDS)", 2: "big_off (sums on demand)"}[form["fused_k4"]]] += nchunks
    if nchunks > form["gx"]:
        ev["K5 a workgroup takes a second chunk"] += nchunks - form["gx"]
    if form["fused_k4"] == 0:
        ev["K4 scan kernel"] += 1
        if nchunks > 8 * THREADS:
            ev["K4 second round of 2048 chunks"] += 1


def _k3_events(ev, seg_bits, raw, form):
    U = len(raw)
    a = np.frombuffer(raw, np.uint8)
    ff = np.zeros(((U + 3) & ~3) + 8, bool)
    ff[:U] = a == 0xFF
    ffw = ff[:(U + 3) & ~3].reshape(-1, 4).any(1)          # word holds an FF byte of the stream
    ln = np.asarray(seg_bits, np.int64)
    nseg = len(ln)
    b1 = np.cumsum(ln)
    b0 = b1 - ln
    wbeg = (b0 + 31) >> 5
    wend = (b1 + 31) >> 5
    wend[-1] = (U + 3) >> 2
    nwords = wend - wbeg
    lead = wbeg * 32 - b0
    slot = form["slot_words"]
    long_seg = ((ln + lead + 31) >> 5) + 2 > slot
    n_int = np.where(ln >= lead + 32, (ln - lead) >> 5, 0)
    edge_bits = np.where(ln > lead, (ln - lead) & 31, 0)
    has_edge = n_int < nwords
    nxt = np.concatenate((ln[1:], [0]))
    has_next = np.arange(nseg) < nseg - 1
    edge_easy = ~has_next | (nxt >= 32 - edge_bits)
    edge_byte0 = (wbeg + n_int) * 4
    edge_valid = np.clip(U - edge_byte0, 0, 4)
    form_name = "long (slot/pool mapping)", "wide", "narrow"
    which = np.where(long_seg, 0, 1 if form["wide"] else 2)
    for k in range(3):
        ev[f"K3 segment placed by the {form_name[k]} path"] += int((which == k).sum())
    ev["K3 empty segment"] += int((ln == 0).sum())
    ev["K3 empty segments follow each other"] += int(((ln[:-1] == 0) & (ln[1:] == 0)).sum())
    ev["K3 segment starts no word of its own"] += int((nwords == 0).sum())
    ev["K3 few-bit segments follow each other"] += int(((ln[:-1] < 32) & (ln[1:] < 32) & (ln[:-1] > 0) & (ln[1:] > 0)).sum())
    for s in np.nonzero(nwords > 0)[0]:
        ev[f"K3 lead = {int(lead[s])}"] += 1
    for s in np.nonzero(has_edge)[0]:
        s = int(s)
        last = s == nseg - 1
        ev[f"K3 edge word holds {int(edge_bits[s])} bits of its segment"] += 1
        # segments whose bits finish the edge word
        lo, hi = int(edge_byte0[s]) * 8, min(int(edge_byte0[s]) * 8 + 32, int(b1[-1]))
        k = int(np.searchsorted(b1, hi, "left")) - s + 1 if hi > lo else 1
        nparts = int(((b1[s:s + max(k, 1) + 1] > lo) & (b0[s:s + max(k, 1) + 1] < hi) & (ln[s:s + max(k, 1) + 1] > 0)).sum())
        if nparts >= 3:
            ev["K3 edge word finished from three or more segments"] += 1
        if not edge_easy[s]:
            ev["K3 edge_easy false: the segment behind is shorter than what the word lacks"] += 1
        ev[f"K3 edge_valid = {int(edge_valid[s])}" + ("" if last else " in an earlier segment's word")] += 1
        for b in range(4):
            if ff[int(edge_byte0[s]) + b]:
                ev[f"K3 FF at byte {b} of an edge word"] += 1
                if last and edge_valid[s] < 4:
                    ev[f"K3 FF in the frame's last word, edge_valid = {int(edge_valid[s])}"] += 1
    # an FF byte made of the bits of two segments
    inner = b1[:-1][(b1[:-1] & 7) != 0]
    inner = inner[(inner >> 3) < U]
    ev["K3 FF byte made of bits of two segments"] += int(ff[inner >> 3].sum())
    words_long = (ln + 31) >> 5
    ev["K3 segment longer than one wave's 768 speculative words"] += int((nwords > WAVE_WORDS).sum())
    ev["K3 segment longer than 1024 words"] += int((words_long > 1024).sum())
    ev["K3 segment longer than its slot"] += int((words_long > slot).sum())
    if form.get("bands"):
        ev["K3 band of exactly 32 * stride bits"] += int((ln == 32 * slot).sum())
        ev["K3 band of 32 * stride - 1 bits"] += int((ln == 32 * slot - 1).sum())
        ev["K3 subs = 1" if form["subs"] == 1 else "K3 subs > 1"] += 1
        ev[f"K3 stride {'< 768' if slot < 768 else '769..775' if 769 <= slot <= 775 else '>= 776' if slot >= 776 else '768'}"] += 1
    if form["wide_subs"]:
        ev["K3 wide_subs: sub-ranges of 768 words"] += 1
    # the 0xFF accounting across a chunk boundary
    for s in np.nonzero((nwords > 0) & ((wbeg >> 10) != ((wend - 1) >> 10)))[0]:
        wb, we = int(wbeg[s]), int(wend[s])
        for bound in range(((wb >> 10) + 1) << 10, we, CHUNK_WORDS):
            if form["wide"] and not long_seg[s]:
                g = wb + 4 * ((bound - wb) // 4)            # the lane's four words g .. g + 3 from wbeg + 4 * lane
                if g < bound < g + 4:
                    ev[f"K3 a lane's four words straddle a chunk boundary, wbeg mod 4 = {wb & 3}"] += 1
                    if ffw[g:bound].any():
                        ev["K3 lane straddles a chunk boundary with FF in front of it"] += 1
                    if ffw[bound:min(g + 4, we)].any():
                        ev["K3 lane straddles a chunk boundary with FF behind it"] += 1
            else:
                i = bound - wb                              # one word per lane: the wave's 64 words from a multiple of 64
                w0 = wb + (i & ~63)
                if w0 < bound:
                    ev["K3 a wave's 64 words straddle a chunk boundary"] += 1
                    if ffw[bound:min(w0 + 64, we)].any():
                        ev["K3 wave straddles a chunk boundary with FF behind it"] += 1
                    if ffw[w0:bound].any():
                        ev["K3 wave straddles a chunk boundary with FF in front of it"] += 1


def _k2_events(ev, seg_bits, form):
    ln = np.asarray(seg_bits, np.int64)
    nseg = len(ln)
    kind = {0: "K2 scan kernel", 1: "K2 inside K3: whole scan in LDS", 2: "K2 inside K3: window of eight, sums on demand"}
    ev[kind[form["fused_k2"]]] += 1
    if form["fused_k2"] == 0:
        ev["K2 clears the chunks' 0xFF counters"] += 1
        if nseg > 8 * THREADS:
            ev["K2 second round of 2048 segments"] += 1
        if form.get("bands"):
            pad = np.concatenate((ln, np.zeros(-nseg % 8, np.int64))).reshape(-1, 8).sum(1)
            rounds = [pad[i:i + THREADS] for i in range(0, len(pad), THREADS)]
            if any(int(r.sum()) >= 1 << 24 for r in rounds):
                ev["K2 two-halves scan: a round's total passes 2^24"] += 1
            if any(int((r >> 24).sum()) > 0 for r in rounds):
                ev["K2 two-halves scan: a thread's run passes 2^24"] += 1


def _k6_events(ev, seg_bits, raw):
    a = np.frombuffer(raw, np.uint8)
    ends = np.cumsum(np.asarray(seg_bits, np.int64))[:-1]
    for e in ends.tolist():
        p = (e >> 3) - 2
        c0 = p // CHUNK * CHUNK
        n = int((a[c0:p] == 0xFF).sum())
        ev[f"K6 placeholder at chunk byte {p % CHUNK}" if p % CHUNK >= CHUNK - 2 or p % CHUNK == 0 else "K6 placeholder inside a chunk"] += 1
        if n >= 2:
            ev["K6 several FF in front of the marker in its chunk"] += 1
        if n >= 2 and p % CHUNK == CHUNK - 1:
            ev["K6 placeholder straddles a chunk boundary with FF in front of it"] += 1


def events(segment_bits, raw_bytes, header_size, form):
    """Counter of the named decision points the stream reaches under `form`"""
    ev = Counter()
    raw = bytes(raw_bytes)
    assert len(raw) == (int(np.sum(segment_bits)) + 7) // 8
    if len(raw) == 0:
        ev["empty stream"] += 1
        return ev
    _k2_events(ev, segment_bits, form)
    _k3_events(ev, segment_bits, raw, form)
    _k5_events(ev, raw, int(np.sum(segment_bits)), header_size, form)
    if form["restart"]:
        _k6_events(ev, segment_bits, raw)
    for k in [k for k, v in ev.items() if v == 0]:
        del ev[k]
    return ev
