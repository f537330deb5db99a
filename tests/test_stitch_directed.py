"""Directed tests of the stitch kernels K2..K6 (sjpeg_amd/csrc/stitch_kernels.h): a designed 0xFF at every byte, edge and
form.  Every case of tests/stitch_cases.py -- the ones whose coverage tests/test_stitch_model_host.py asserts on the
model's events -- goes through its route and is compared byte for byte, size included, with the plain stitch of
tests/stitch_model.py; a failure names the place in the stream (chunk, group, byte, word, segment) and what the model
sees there.  Every output lies in a buffer of guard bytes that must come back untouched.

Which kernel form a route takes is worked out by tests/stitch_model.py (the library cannot be asked).  The `big_off` step
of fused form 2 to a workgroup's second chunk needs a frame above 4096 chunks and stays with the 8K digest test of
test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import entropy_model as em
import sjpeg_amd as sj
import stitch_cases as sc
import stitch_model as sm

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


# ---------------------------------------------------------------------------------------------- naming the place

def form_text(form):
    return (f"place_segments<{form['fused_k2']}{', RAGGED' if form['ragged'] else ''}> {'wide' if form['wide'] else 'narrow'} form"
            f"{', wide_subs' if form['wide_subs'] else ''}, stuff_chunks<{form['fused_k4']}{', RAGGED' if form['ragged'] else ''}>")


def where(got, want, raw, hlen, seg_bits=None, form=None):
    """the first byte at which got and want differ, as a place of the un-stuffed stream, with the model's events there"""
    got, want = bytes(got), bytes(want)
    if got == want:
        return "equal"
    if form is not None:
        return form_text(form) + ": " + where(got, want, raw, hlen, seg_bits)
    n = min(len(got), len(want))
    i = next((k for k in range(n) if got[k] != want[k]), n)
    text = f"sizes {len(got)} / {len(want)}, first difference at output byte {i}"
    if i < hlen:
        return text + " (header)"
    a = np.frombuffer(bytes(raw), np.uint8)
    at = np.arange(len(a)) + np.concatenate(([0], np.cumsum(a == 0xFF)[:-1]))     # stuffed position of every raw byte
    r = int(np.searchsorted(at, i - hlen, "right")) - 1
    if r >= len(a) or r < 0:
        return text + " (behind the stream: EOI / size)"
    g0 = r // 16 * 16
    ffs = lambda lo, hi: [k - lo for k in range(lo, min(hi, len(a))) if a[k] == 0xFF]
    text += (f": stream byte {r} = chunk {r // sm.CHUNK}, thread {r % sm.CHUNK // 16}, byte {r % 16} of its group; "
             f"0xFF in the group at {ffs(g0, g0 + 16)}, in front at {ffs(max(g0 - 16, 0), g0)}, in the first four behind at "
             f"{ffs(g0 + 16, g0 + 20)}; word {r // 4}")
    # the model's events of that group (tests/stitch_model.py)
    own, beh = ffs(g0, g0 + 16), ffs(g0 + 16, g0 + 20)
    state = "plain" if not beh else f"ff@{beh[0]}" if len(beh) == 1 else "several FF"
    slow = bool(own) or any(b < 3 for b in beh) or g0 + 16 > len(a)
    text += (f"; event: K5 group: {'ff@%d' % own[0] if len(own) == 1 else 'plain' if not own else 'several FF'} behind {state} "
             f"({'slow' if slow else 'fast'} thread, {'slow' if ffs(max(g0 - 16, 0), g0) or own[:1] and own[0] < 3 else 'fast'} "
             "thread in front)")
    if seg_bits is not None:
        b1 = np.cumsum(np.asarray(seg_bits, np.int64))
        s = int(np.searchsorted(b1, 8 * r, "right"))
        s = min(s, len(b1) - 1)
        b0 = int(b1[s] - seg_bits[s])
        text += (f", segment {s} of {len(b1)} (bits {b0}..{int(b1[s])}: lead {(-b0) % 32}, word {(r // 4) - (b0 + 31) // 32} "
                 f"of its {(int(b1[s]) + 31) // 32 - (b0 + 31) // 32}, ends in word {int(b1[s]) // 32})")
        if r // 4 == int(b1[s]) // 32 and int(b1[s]) % 32:
            nxt = int(seg_bits[s + 1]) if s + 1 < len(b1) else None
            text += (f"; event: K3 edge word holds {int(b1[s]) % 32} bits of its segment, edge_valid = {min(4, len(a) - r // 4 * 4)}, "
                     f"edge_easy {nxt is None or nxt >= 32 - int(b1[s]) % 32}")
    return text


def guarded(nbytes):
    buf = torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[PAD:PAD + nbytes]


def untouched(buf, used):
    """every byte of buf outside the ranges `used` (relative to the output's start) still holds the guard"""
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for lo, hi in used:
        mask[PAD + lo:PAD + hi] = False
    return bool((buf[mask] == GUARD).all().item())


# ---------------------------------------------------------------------------------------------- bands

def run_bands(engine, case, cap, words=None):
    """sjpeg_hip_stitch_bands into a guarded buffer of exactly `cap` bytes -> (bytes, buffer intact)"""
    w = torch.from_numpy(case.words()).cuda() if words is None else words
    nbits = torch.tensor(case.lens, dtype=torch.int64, device="cuda")
    buf, out = guarded(cap)
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = sj.lib().sjpeg_hip_stitch_bands(engine._h, len(case.lens), w.data_ptr(), case.stride, nbits.data_ptr(), case.header,
                                         len(case.header), 1, out.data_ptr(), cap, size.data_ptr(), engine._stream())
    assert rc == 0, sj.lib().sjpeg_hip_last_error().decode()
    n = int(size.item())
    return bytes(out[:n].cpu().numpy()), untouched(buf, [(0, n)])


BAND_GROUPS = {"pairs": "pairs-", "runs": ("runs", "chunk-of-ff", "two-chunks"), "lengths": "U", "short": ("short", "lead"),
               "strides": "full-bands", "scans": ("2100", "ten-bands")}


@pytest.mark.parametrize("group", list(BAND_GROUPS))
def test_bands(engine, group):
    cases = [c for c in sc.band_cases() if c.name.startswith(BAND_GROUPS[group])]
    assert cases
    for c in cases:
        raw = sm.raw_stream(c.bands())[0]
        # (the plain stitch byte by byte; the two streams of megabytes with bytes.replace)
        want = sm.stitch(c.bands(), c.header) if len(raw) < 1 << 18 else c.header + raw.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
        floor = len(c.header) + 2 + 64                      # (the entry refuses a smaller buffer)
        got, intact = run_bands(engine, c, max(len(want), floor))
        assert got == want, (c.name, where(got, want, raw, len(c.header), c.lens, c.form()))
        assert intact, (c.name, "guard bytes written")
        if len(want) > floor:                               # one byte short: size 0, nothing written
            got, intact = run_bands(engine, c, len(want) - 1)
            assert got == b"" and intact, (c.name, "one byte short")


def test_bands_of_a_stream_of_more_than_4096_chunks(engine):
    """a workgroup of the band entry takes a second chunk; K4 scans in three rounds.  Built with numpy, checked with
    bytes.replace."""
    c = sc.big_band_case()
    raw = bytes(c._raw[:-1]) + bytes([int(c._raw[-1]) | 7])
    want = raw.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    bits = np.unpackbits(c._raw)
    words = np.zeros((len(c.lens), c.stride), np.int32)
    at = 0
    for i, n in enumerate(c.lens):
        words[i] = sm.words_of(bits[at:at + n], c.stride)
        at += n
    del bits
    got, intact = run_bands(engine, c, len(want), words=torch.from_numpy(words).cuda())
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, where(got, want, raw, 0, c.lens, c.form())
    assert intact


# ---------------------------------------------------------------------------------------------- pictures

class Loaded:
    def __init__(self, pic, oracle):
        self.pic, self.name = pic, pic.name
        self.case = case = pic.case(oracle)
        self.frames = torch.from_numpy(case.rgb).cuda().unsqueeze(0)
        self.planes = [self.frames[0].view(case.h, case.w * 3)]
        self.dc, self.ac = pic.codes()
        self.symbols = case.symbols(oracle)
        body, tr = em.encode_symbols(self.symbols, self.dc, self.ac)
        self.body, self.trace, self.seg = body, tr, tr.segment_bits
        self.raw = body.replace(b"\xff\x00", b"\xff")
        tables0, self.quant = sj.make_tables(quant=case.quant)
        self._tables0 = tables0
        self.header = sj.make_header_ex(case.w, case.h, case.yuv_mode, self.quant, em.huffman_specs(sj, self.dc, self.ac))
        self.want = self.header + body + b"\xff\xd9"

    def tables(self, flags=0):
        t = sj.ScanTables()
        C.memmove(C.byref(t), C.byref(self._tables0), C.sizeof(t))
        for c in range(2):
            t.dc_codes[c][:] = [int(v) for v in self.dc[c]]
            t.ac_codes[c][:] = [int(v) for v in self.ac[c]]
        t.flags = flags
        return t

    def key(self):
        return (self.case.w, self.case.h, id(self.dc), self.case.quant.tobytes())

    def say(self, got, want=None, header=None, form=None):
        return self.name, where(got, self.want if want is None else want, self.raw, len(self.header if header is None else header),
                                self.seg, form)


@pytest.fixture(scope="module")
def loaded(oracle):
    return [Loaded(p, oracle) for p in sc.pictures()]


@pytest.mark.parametrize("route", ["fused 1, tight", "fused 1", "fused 2"])
def test_uniform_entry_one_frame(engine, loaded, route):
    """sjpeg_hip_encode_scan: K2 and K4 inside K3 and K5 (form 1, at an exact-fit and at a 1 MiB out_stride) and the
    large form 2 (12 MiB)"""
    for p in loaded:
        routes = sc.uniform_routes(p.pic, len(p.want), len(p.header))
        if route not in routes:                             # (form 2 needs 158 segments: the main ruler)
            assert route == "fused 2" and p.pic.nseg < 158
            continue
        stride, form = routes[route]
        assert (form["fused_k2"], form["fused_k4"]) == ((2, 2) if route == "fused 2" else (1, 1))
        buf, out = guarded(stride)
        sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
        engine.encode_frames(p.frames, p.tables(), p.header, em.YUV_400, out=out.view(1, stride), sizes=sizes, out_stride=stride)
        n = int(sizes[0].item())
        got = bytes(out[:n].cpu().numpy())
        assert got == p.want, (route, *p.say(got, form=form))
        assert untouched(buf, [(0, n)]), (route, p.name, "guard bytes written")


def _batches(loaded, n):
    """the pictures in batches of n frames of one size and one table set, every picture in at least one"""
    groups = {}
    for p in loaded:
        groups.setdefault(p.key(), []).append(p)
    out = []
    for g in groups.values():
        for lo in range(0, len(g), n):
            out.append([g[(lo + k) % len(g)] for k in range(n)])
    return out


def test_uniform_entry_packed_four_frames(engine, loaded):
    """sjpeg_hip_encode_scan_packed_src: K2, K4 as kernels (form 0), the frames' places from pack_off"""
    for batch in _batches(loaded, 4):
        p0 = batch[0]
        stride = sc.FUSED1_STRIDE if len(p0.want) <= sc.FUSED1_STRIDE else sc.tight(len(p0.want))
        assert sm.uniform_form(4, p0.pic.nseg, stride, packed=True)["fused_k4"] == 0
        frames = torch.cat([p.frames for p in batch])
        buf, out = guarded(4 * stride)
        sizes = torch.zeros(4, dtype=torch.int64, device="cuda")
        offsets = torch.zeros(5, dtype=torch.int64, device="cuda")
        engine.encode_frames_packed(frames, p0.tables(), p0.header, em.YUV_400, out, sizes, offsets, stride)
        sz, off = sizes.cpu().numpy().tolist(), offsets.cpu().numpy().tolist()
        host = out[:off[4]].cpu().numpy()
        at = 0
        for k, p in enumerate(batch):
            got = host[off[k]:off[k] + sz[k]].tobytes()
            assert off[k] == at and got == p.want, ("packed", k, *p.say(got, form=sm.uniform_form(4, p0.pic.nseg, stride, packed=True)))
            at = sc.tight(off[k] + sz[k])
            assert (host[off[k] + sz[k]:at] == 0).all(), ("packed: padding", p.name)
        assert off[4] == at and untouched(buf, [(0, at)]), ("packed", p0.name, "guard bytes written")


def test_uniform_entry_per_frame_tables_and_headers(engine, loaded):
    """sjpeg_hip_encode_scan_multi: form 1 with hdr_off -- three frames whose headers differ in length by 5 and 11 bytes,
    so that the frames' first chunks land at three misalignments"""
    for batch in _batches(loaded, 3):
        p0 = batch[0]
        n, w, h = 3, p0.case.w, p0.case.h
        headers = [p.header + bytes(range(1, 1 + 5 * k + k * k)) for k, p in enumerate(batch)]
        wants = [hd + p.body + b"\xff\xd9" for hd, p in zip(headers, batch)]
        stride = sc.FUSED1_STRIDE if max(map(len, wants)) <= sc.FUSED1_STRIDE else sc.tight(max(map(len, wants)))
        assert sm.uniform_form(3, p0.pic.nseg, stride)["fused_k4"] == 1
        frames = torch.cat([p.frames for p in batch])
        src, _keep = sj.make_source(sj.SRC_RGB, [frames.view(n, h, w * 3)])
        arr = (sj.ScanTables * n)(*[p.tables() for p in batch])
        offs = (C.c_size_t * (n + 1))()
        for i, hd in enumerate(headers):
            offs[i + 1] = offs[i] + len(hd)
        buf, out = guarded(n * stride)
        sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        rc = sj.lib().sjpeg_hip_encode_scan_multi(engine._h, C.byref(src), w, h, em.YUV_400, n, C.cast(arr, C.c_void_p),
                                                  b"".join(headers), offs, 1, out.data_ptr(), stride, sizes.data_ptr(),
                                                  engine._stream())
        assert rc == 0, sj.lib().sjpeg_hip_last_error().decode()
        sz = sizes.cpu().numpy().tolist()
        used = []
        for k, p in enumerate(batch):
            got = bytes(out[k * stride:k * stride + sz[k]].cpu().numpy())
            assert got == wants[k], ("multi", k, *p.say(got, wants[k], headers[k], sm.uniform_form(3, p0.pic.nseg, stride)))
            used.append((k * stride, k * stride + sz[k]))
        assert untouched(buf, used), ("multi", p0.name, "guard bytes written")


@pytest.mark.parametrize("short", [0, 1])
def test_ragged_entry_all_pictures_at_exact_capacities(engine, loaded, short):
    """sjpeg_hip_encode_ragged_src, mixed sizes, per-frame tables: the ragged forms <0, true>, one wave a segment.  The
    exact capacity gives the bytes -- the flat pictures' last byte is a stuffed FF --, one byte less gives size 0."""
    caps = [len(p.want) - short for p in loaded]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += sc.tight(c) + 48
    buf, out = guarded(at)
    _, sizes, _ = engine.encode_ragged(sj.SRC_RGB, [p.planes for p in loaded], [(p.case.w, p.case.h) for p in loaded],
                                       em.YUV_400, [p.tables() for p in loaded], [p.header for p in loaded],
                                       capacities=caps, out=out, offsets=offs)
    sz = sizes.cpu().numpy().tolist()
    host = out.cpu().numpy()
    for k, p in enumerate(loaded):
        got = host[offs[k]:offs[k] + sz[k]].tobytes()
        if short:
            assert sz[k] == 0, ("ragged, one byte short", p.name, sz[k])
        else:
            assert got == p.want, ("ragged", *p.say(got, form=sm.ragged_form(caps, [q.pic.nseg for q in loaded], k)))
    assert untouched(buf, [(o, o + s) for o, s in zip(offs, sz)]), ("ragged", short, "guard bytes written")


def test_counted_bits_of_the_rulers(engine, loaded):
    """K1..K3 + counted_bits_ragged: the padded last byte FF (flat pictures of 3 and 11 blocks: taken off again) and not"""
    got = engine.scan_counted_bits_ragged(sj.SRC_RGB, [p.planes for p in loaded], [(p.case.w, p.case.h) for p in loaded],
                                          em.YUV_400, [p.tables() for p in loaded]).cpu().numpy().tolist()
    for p, g in zip(loaded, got):
        assert g == p.trace.counted_bits, (p.name, g, p.trace.counted_bits, "padded last byte",
                                           hex(p.raw[-1]), "T mod 8 =", p.trace.total_bits % 8)
    names = {p.name: p for p in loaded}
    assert names["ruler-flat-3"].raw[-1] == 0xFF and names["ruler-flat-11"].raw[-1] == 0xFF and names["ruler-main"].raw[-1] != 0xFF


def test_restart_markers_at_a_chunk_boundary(engine, oracle):
    """K6: a marker whose placeholder lies at chunk bytes 4095 | 0, the intervals' leading 0xFF bytes in front of it"""
    r = sc.restart_ruler()
    p = Loaded(r, oracle)
    body, raws = sm.encode_restart(p.case.coeffs(oracle), em.YUV_400, p.dc, p.ac)
    seg, raw = sm.restart_stream(raws)
    ev = sm.events(seg, raw, 0, sm.uniform_form(1, r.nseg, sc.FUSED1_STRIDE, restart=True))
    assert ev["K6 placeholder straddles a chunk boundary with FF in front of it"] > 0
    header = sj.header_add_restart(p.header, em.YUV_400)
    want = header + body + b"\xff\xd9"
    stride = sc.FUSED1_STRIDE
    buf, out = guarded(stride)
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    engine.encode_frames(p.frames, p.tables(sj.RESTART_MARKERS), header, em.YUV_400, out=out.view(1, stride), sizes=sizes,
                         out_stride=stride)
    n = int(sizes[0].item())
    got = bytes(out[:n].cpu().numpy())
    # (the markers are bytes of the output, not of the stitch's stream: placeholders stand for them in `raw`)
    ends = (np.cumsum(seg)[:-1] >> 3) - 2
    assert got == want, ("restart: patch_restart_markers", where(got, want, raw, len(header), seg, sm.uniform_form(1, r.nseg, stride, restart=True)),
                         "placeholders at chunk bytes", sorted(set((ends % sm.CHUNK).tolist()))[-3:])
    assert untouched(buf, [(0, n)])


# ---------------------------------------------------------------------------------------------- 64 frames

@pytest.fixture(scope="module")
def noise(oracle):
    c = sc.saturated_noise()
    tables, quant = sj.make_tables(quant=c.quant)
    header = sj.make_header(c.w, c.h, em.YUV_400, quant)
    want = oracle.encode_matrices(c.rgb, c.quant, yuv_mode=em.YUV_400)
    body = em.scan_body(want)
    assert want == header + body + b"\xff\xd9"
    raw = body.replace(b"\xff\x00", b"\xff")
    assert len(raw) >= 66 * sm.CHUNK
    return c, tables, header, want, raw


def test_ragged_64_frames_second_chunk_of_a_workgroup(engine, oracle, noise):
    """63 pictures of 8 x 8 beside the saturated-noise frame: 64 workgroups of K5 for its 94 chunks"""
    c, tables, header, want, raw = noise
    small = [np.repeat(np.random.RandomState(k).randint(0, 256, (8, 8, 1)).astype(np.uint8), 3, 2) for k in range(63)]
    imgs = small[:31] + [c.rgb] + small[31:]
    wants = [want if im is c.rgb else oracle.encode_matrices(im, c.quant, yuv_mode=em.YUV_400) for im in imgs]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    headers = [header if im is c.rgb else sj.make_header(8, 8, em.YUV_400, sj.make_tables(quant=c.quant)[1]) for im in imgs]
    caps = [len(w) for w in wants]
    offs, at = [], 0
    for cp in caps:
        offs.append(at)
        at += sc.tight(cp) + 48
    buf, out = guarded(at)
    _, sizes, _ = engine.encode_ragged(sj.SRC_RGB, [[d.view(d.shape[0], -1)] for d in dev], [(im.shape[1], im.shape[0]) for im in imgs],
                                       em.YUV_400, [tables] * 64, headers, capacities=caps, out=out, offsets=offs)
    sz = sizes.cpu().numpy().tolist()
    host = out.cpu().numpy()
    for k in range(64):
        got = host[offs[k]:offs[k] + sz[k]].tobytes()
        assert got == wants[k], ("ragged 64", k, where(got, wants[k], raw, len(header), None, sm.ragged_form(caps, [1] * 31 + [16] + [1] * 32, 31)) if k == 31 else (len(got), len(wants[k])))
    assert untouched(buf, [(o, o + s) for o, s in zip(offs, sz)])


def test_uniform_packed_64_frames_second_chunk_of_a_workgroup(engine, noise):
    """gx = 64 workgroups a frame, 94 chunks: form 0 with pack_off, the second chunk's offset from co[]"""
    c, tables, header, want, raw = noise
    stride = sc.tight(len(want) + 100)
    f = sm.uniform_form(64, 16, stride, packed=True)
    assert f["gx"] == 64 and f["fused_k4"] == 0 and -(-len(raw) // sm.CHUNK) > 64
    frames = torch.from_numpy(c.rgb).cuda().unsqueeze(0).expand(64, -1, -1, -1).contiguous()
    buf, out = guarded(64 * stride)
    sizes = torch.zeros(64, dtype=torch.int64, device="cuda")
    offsets = torch.zeros(65, dtype=torch.int64, device="cuda")
    engine.encode_frames_packed(frames, tables, header, em.YUV_400, out, sizes, offsets, stride)
    sz, off = sizes.cpu().numpy().tolist(), offsets.cpu().numpy().tolist()
    host = out[:off[64]].cpu().numpy()
    step = sc.tight(len(want))
    for k in range(64):
        got = host[off[k]:off[k] + sz[k]].tobytes()
        assert off[k] == k * step and got == want, ("packed 64", k, where(got, want, raw, len(header), None, f))
    assert off[64] == 64 * step and untouched(buf, [(0, off[64])])


def test_ragged_packed_saturated_noise_against_the_oracle(engine, oracle):
    """sjpeg_hip_encode_ragged_packed_src takes no caller's tables: the rulers cannot go through it.  The saturated-noise
    frame between two small ones, against the oracle alone."""
    c = sc.saturated_noise()
    small = np.repeat(np.random.RandomState(3).randint(0, 256, (16, 24, 1)).astype(np.uint8), 3, 2)
    imgs = [small, c.rgb, small]
    wants = [oracle.encode_full(im, c.quant, yuv_mode=em.YUV_400, method=0) for im in imgs]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    total = sum(sc.tight(len(w)) for w in wants)
    buf, out = guarded(total)
    res = engine.encode_ragged_packed(sj.SRC_RGB, [[d.view(d.shape[0], -1)] for d in dev], [(im.shape[1], im.shape[0]) for im in imgs],
                                      em.YUV_400, c.quant, 0, capacities=[len(w) for w in wants], packed_capacity=total, out=out)
    engine.wait()
    torch.cuda.synchronize()
    sz, off = res[1].cpu().numpy().tolist(), res[2].cpu().numpy().tolist()
    host = out.cpu().numpy()
    for k in range(3):
        got = host[off[k]:off[k] + sz[k]].tobytes()
        assert got == wants[k], ("ragged packed", k, len(got), len(wants[k]))
    assert off[3] == total and untouched(buf, [(0, total)])
