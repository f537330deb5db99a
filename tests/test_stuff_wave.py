"""stuff_chunks_wave (sjpeg_amd/csrc/stitch_kernels.h): K5 of every launch that is not fused -- one wave per 4 KiB chunk,
every lane writing its own 16 bytes and the 0x00 behind its 0xFF bytes straight to the output.  The designs of
tests/stitch_cases.py through the three routes that reach it with small inputs: the band entry (arbitrary bit streams:
an FF at every byte of a group beside every state of its neighbour, runs across sub-block and chunk boundaries, a chunk
of FF, streams of 1..17 bytes and of 4096 k, k +- 1, every misalignment of the chunks), the packed uniform entry with four
frames (the rulers, placed through pack_off) and the engine in pipelined mode (a 64 x 64 and a 640 x 480 picture, two
calls in flight).  Everything byte for byte against the plain stitch of tests/stitch_model.py or the oracle, in buffers of
guard bytes that must come back untouched: no lane stores past its last byte.  The kernel's lane code runs on the CPU,
store by store, in tests/test_stuff_wave_cxx.py."""
import numpy as np
import pytest
import torch

import entropy_model as em
import sjpeg_amd as sj
import stitch_cases as sc
import stitch_model as sm
from test_stitch_directed import Loaded, guarded, run_bands, untouched, where

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


BAND_GROUPS = {"pairs at every misalignment": "pairs-", "runs and chunks of FF": ("runs", "chunk-of-ff", "two-chunks"),
               "stream lengths": "U"}


@pytest.mark.parametrize("group", list(BAND_GROUPS))
def test_band_entry(engine, group):
    cases = [c for c in sc.band_cases() if c.name.startswith(BAND_GROUPS[group])]
    assert cases
    for c in cases:
        assert c.form()["fused_k4"] == 0
        raw = sm.raw_stream(c.bands())[0]
        want = sm.stitch(c.bands(), c.header)
        got, intact = run_bands(engine, c, max(len(want), len(c.header) + 2 + 64))
        assert got == want, (c.name, where(got, want, raw, len(c.header), c.lens, c.form()))
        assert intact, (c.name, "guard bytes written")


def test_packed_entry_four_small_frames(engine, oracle):
    """the rulers of up to 1024 x 1056 pixels in batches of four frames of one size: form 0, the frames' places from pack_off"""
    loaded = [Loaded(p, oracle) for p in sc.rulers()[1:] + sc.tail_rulers()[:5] + sc.flat_rulers()]
    groups = {}
    for p in loaded:
        groups.setdefault(p.key(), []).append(p)
    for g in groups.values():
        batch = [g[k % len(g)] for k in range(4)]
        p0 = batch[0]
        stride = sc.FUSED1_STRIDE
        form = sm.uniform_form(4, p0.pic.nseg, stride, packed=True)
        assert form["fused_k4"] == 0 and max(len(p.want) for p in batch) <= stride
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
            assert off[k] == at and got == p.want, ("packed", k, *p.say(got, form=form))
            at = sc.tight(off[k] + sz[k])
            assert (host[off[k] + sz[k]:at] == 0).all(), ("packed: padding", p.name)
        assert off[4] == at and untouched(buf, [(0, at)]), ("packed", p0.name, "guard bytes written")


@pytest.mark.parametrize("w,h,mode,quality", [(64, 64, sj.YUV_400, 50.0), (640, 480, sj.YUV_420, 75.0)])
def test_pipelined_engine_on_small_pictures(oracle, w, h, mode, quality):
    """pipelined mode never fuses K4 into K5: two calls back to back, two frames each, against the oracle"""
    from oracle import synth
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    imgs = [synth.g_struct(w, h, 7654321), synth.g_noise(w, h, 1234567)]
    wants = [oracle.encode(im, quality, mode) for im in imgs]
    tables, q = sj.make_tables(quality=quality)
    header = sj.make_header(w, h, mode, q)
    stride = sc.tight(max(len(x) for x in wants) + 200)
    runs = []
    for order in ((0, 1), (1, 0)):
        frames = torch.from_numpy(np.stack([imgs[i] for i in order])).cuda()
        buf, out = guarded(2 * stride)
        sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
        eng.encode_frames(frames, tables, header, mode, out=out.view(2, stride), sizes=sizes, out_stride=stride)
        runs.append((order, frames, buf, out, sizes))
    eng.wait()
    torch.cuda.synchronize()
    for order, _, buf, out, sizes in runs:
        sz = sizes.cpu().numpy().tolist()
        for k, i in enumerate(order):
            got = bytes(out[k * stride:k * stride + sz[k]].cpu().numpy())
            assert got == wants[i], (order, k, len(got), len(wants[i]))
        assert untouched(buf, [(k * stride, k * stride + sz[k]) for k in range(2)]), (order, "guard bytes written")
    eng.close()
