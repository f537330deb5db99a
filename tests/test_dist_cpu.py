"""world_size-2 gloo test of the multi-GPU plumbing (sjpeg_amd/dist.py): frame sharding and the
gather of variable-length coded frames to rank 0.  Payloads are oracle-coded frames so the
assembled batch is checked against the real expected bytes.  CPU only."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compact_torch(out, sizes, n, capacity):
    """What sjpeg_hip_compact_streams does (include/sjpeg_hip.h), restated with torch ops for the
    CPU tests: frames back to back, every one at a multiple of 16, padding zero."""
    offs = [0]
    for i in range(n):
        offs.append(offs[-1] + ((int(sizes[i]) + 15) & ~15))
    packed = torch.zeros(int(capacity), dtype=torch.uint8)
    for i in range(n):
        packed[offs[i]:offs[i] + int(sizes[i])] = out[i, :int(sizes[i])]
    return packed, torch.tensor(offs, dtype=torch.int64)


def _worker(rank, world, port, nframes, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import orc, synth
    from sjpeg_amd.dist import gather_streams, shard_frames
    o = orc.oracle()
    ids = shard_frames(nframes, rank, world)
    coded = [o.encode(synth.g_struct(48, 40, 100 + k), 75.0, 1) for k in ids]
    stride = max([len(c) for c in coded] + [1]) + 13
    out = torch.zeros((max(len(ids), 1), stride), dtype=torch.uint8)
    sizes = torch.zeros(max(len(ids), 1), dtype=torch.int64)
    for i, c in enumerate(coded):
        out[i, :len(c)] = torch.from_numpy(np.frombuffer(c, np.uint8).copy())
        sizes[i] = len(c)
    frames = gather_streams(out, sizes, ids, nframes, dst=0, compact=_compact_torch)
    if rank == 0:
        want = [o.encode(synth.g_struct(48, 40, 100 + k), 75.0, 1) for k in range(nframes)]
        q.put(frames == want)
    else:
        assert frames is None
    dist.barrier()
    dist.destroy_process_group()


def _run(nframes):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, nframes, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok


def _worker_lost(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sjpeg_amd as sj
    from sjpeg_amd.dist import gather_streams, shard_frames
    ids = shard_frames(4, rank, world)
    out = torch.full((2, 64), 7, dtype=torch.uint8)
    sizes = torch.tensor([40, 0 if rank == 1 else 33], dtype=torch.int64)   # rank 1's second frame did not fit its slot
    try:
        gather_streams(out, sizes, ids, 4, dst=0, compact=_compact_torch)
        q.put((rank, "no error"))
    except sj.SjpegError as e:
        q.put((rank, "refused" if "size 0" in str(e) else str(e)))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_refuses_a_lost_frame_on_every_rank():
    """A frame of size 0 (it did not fit its slot) must not become an empty string in the gathered batch:
    every rank sees it in the rows and raises before anything is sent (nobody is left waiting)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker_lost, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == {0: "refused", 1: "refused"}


def test_shard_assignment():
    from sjpeg_amd.dist import shard_frames
    assert shard_frames(64, 3, 8) == list(range(3, 64, 8))
    assert sorted(sum((shard_frames(7, r, 2) for r in range(2)), [])) == list(range(7))
    assert shard_frames(1, 1, 2) == []


def test_gather_even():
    _run(6)


def test_gather_ragged_and_empty_rank():
    _run(5)
    _run(1)


def _loop_worker(rank, world, port, nframes, nsteps, q, shrink=False):
    """bench.py's multi-rank region (sjpeg_amd.dist.exchange_loop) with a stand-in encoder: step s
    leaves the oracle-coded frames of picture set s in buffer set s & 1."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import orc, synth
    from sjpeg_amd.dist import exchange_loop, shard_frames
    o = orc.oracle()
    ids = shard_frames(nframes, rank, world)

    def coded(step, k):
        # (shrink: every step's streams are shorter than the step before -- a result that shared its buffer with
        # step s + 2 would read that step's bytes)
        wide = (40 + 8 * (k % 3)) if not shrink else (88 - 16 * step + 8 * (k % 3))
        return o.encode(synth.g_struct(wide, 24, 1000 * step + k), 75.0, 1)

    stride = 4096
    outs = [torch.zeros((max(len(ids), 1), stride), dtype=torch.uint8) for _ in range(2)]
    sizes = [torch.zeros(max(len(ids), 1), dtype=torch.int64) for _ in range(2)]
    state = {"step": 0}

    def encode(b):
        for i, k in enumerate(ids):
            c = coded(state["step"], k)
            outs[b][i].zero_()
            outs[b][i, :len(c)] = torch.from_numpy(np.frombuffer(c, np.uint8).copy())
            sizes[b][i] = len(c)
        state["step"] += 1

    got = exchange_loop(nsteps, encode, outs, sizes, ids, nframes, use_streams=False, compact=_compact_torch)
    if rank == 0:
        ok = len(got) == nsteps
        for s, g in enumerate(got):
            ok = ok and g.frames() == [coded(s, k) for k in range(nframes)]
        q.put(ok)
    else:
        assert got == [None] * nsteps
    dist.barrier()
    dist.destroy_process_group()


def test_bench_exchange_loop_two_ranks():
    """Exactly the code path of `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`
    between its two fences, on gloo."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_loop_worker, args=(r, 2, port, 5, 3, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok


def test_exchange_loop_keeps_every_step_when_later_steps_are_smaller():
    """keep="all": the result of step s must survive step s + 2, which reuses the same output set and scratch
    and gathers FEWER bytes (the gathered buffer was shared)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_loop_worker, args=(r, 2, port, 5, 4, q, True)) for r in range(2)]
    for p in procs:
        p.start()
    ok = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok


def _packed_loop_worker(rank, world, port, nframes, nsteps, q):
    """exchange_loop with PACKED output sets (what Engine.encode_frames_packed leaves: a flat buffer + offsets):
    no compaction pass, and rank 0 as the root receives the others BEHIND its own streams in that very buffer."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import orc, synth
    from sjpeg_amd.dist import exchange_loop, shard_frames
    o = orc.oracle()
    ids = shard_frames(nframes, rank, world)

    def coded(step, k):
        return o.encode(synth.g_struct(40 + 8 * (k % 3), 24, 1000 * step + k), 75.0, 1)

    room = 1 << 16                                       # long enough for the whole world's streams
    outs = [torch.full((room,), 0x5A, dtype=torch.uint8) for _ in range(2)]
    sizes = [torch.zeros(max(len(ids), 1), dtype=torch.int64) for _ in range(2)]
    poffs = [torch.zeros(len(ids) + 1, dtype=torch.int64) for _ in range(2)]
    state = {"step": 0}

    def encode(b):
        at = 0
        for i, k in enumerate(ids):
            c = coded(state["step"], k)
            poffs[b][i] = at
            outs[b][at:at + ((len(c) + 15) & ~15)] = 0
            outs[b][at:at + len(c)] = torch.from_numpy(np.frombuffer(c, np.uint8).copy())
            sizes[b][i] = len(c)
            at += (len(c) + 15) & ~15
        poffs[b][len(ids)] = at
        state["step"] += 1

    got = exchange_loop(nsteps, encode, outs, sizes, ids, nframes, use_streams=False, compact=None, keep="last",
                        packed_offsets=poffs)
    if rank == 0:
        g = got[-1]
        ok = len(got) == 1 and g.frames() == [coded(nsteps - 1, k) for k in range(nframes)]
        # in place: the gathered buffer IS the root's own output set of the last step
        ok = ok and g.gathered.data_ptr() == outs[(nsteps - 1) & 1].data_ptr()
        q.put(ok)
    else:
        assert got == [None]
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_loop_with_packed_output_and_the_root_in_place():
    """packed_offsets was honoured on the CUDA path only -- on gloo the already-packed buffer was
    compacted a second time with the wrong stride."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_packed_loop_worker, args=(r, 2, port, 5, 3, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok


def test_bench_launcher_starts_the_world_it_was_asked_for():
    """`python bench.py --gpus 2` without a torch.distributed environment must start two ranks by itself
    (the flag was parsed and ignored).  --launch-check takes the launcher's exact path -- a child
    torch.distributed.run on 127.0.0.1 -- and meets on gloo instead of touching a device."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                                   # ONE line, from rank 0
    got = json.loads(lines[0])
    assert got["n_gpus"] == 2 and got["ranks"] == [0, 1]
    # one rank: no launcher, same line shape
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--launch-check"],
                        capture_output=True, text=True, timeout=300, env=env)
    assert r1.returncode == 0 and json.loads([ln for ln in r1.stdout.splitlines() if ln.startswith("{")][0])["n_gpus"] == 1


def test_bench_two_ranks_end_to_end_with_a_stand_in_device():
    """`bench.py --gpus 2` from `import torch` to the JSON line on gloo: the process group, the fences
    and max-over-ranks timing, the packed-output exchange loop, the local sinks, config #4 sharded + gathered with
    its real MD5 check, the model of the two ceilings -- everything but the device (tests/bench_stub.py: CPU tensors
    for "cuda" ones, an engine that writes the oracle's streams).  The first run on an 8-GPU node must not be the
    first run of this code."""
    import json
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "tests", "bench_stub.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--regions", "2", "--frames", "3", "--input", "noise", "--no-cpu-baseline", "--full"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                           # ONE line, from rank 0
    d = json.loads(lines[0])
    assert d["stub"] is True and d["value"] == 0.0                     # never mistaken for a measurement
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["bit_exact"] is True and "error" not in d
    for key in ("metric", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["with_gather"]["verified"] is True and d["with_gather"]["value"] > 0
    assert d["with_local_sink"]["verified"] is True and d["with_local_sink"]["value"] > 0
    c4 = d["c4_sharded_gathered"]
    assert c4["bit_exact"] is True and c4["frames_per_rank"] == 32 and c4["gathered_bytes_per_step"] == 33508705
    assert c4["encode_only"]["mpix_s"] > 0 and c4["with_gather"]["mpix_s"] > 0
    m = d["multi_gpu_model"]
    assert m["quote_beside_value"] == "with_local_sink" and m["rooted_gather_ceiling_per_peer_mpix_s"] > 0


def test_bench_dump_outputs_with_a_stand_in_device(tmp_path):
    """`bench.py --dump-outputs DIR` (one rank, the stand-in device of tests/bench_stub.py): what the last timed step
    returned, as float arrays -- the sizes and checksums of the oracle's streams --, and the same files again from a
    second run with the same arguments."""
    import json
    import subprocess
    from oracle import orc, synth
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_stub.py"), "--gpus", "1", "--steps", "2",
                            "--warmup", "1", "--frames", "3", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 2 and line["regions"] == 1 and "other_configs" not in line and "cpu_baseline" not in line
        got = {n: np.load(d / f"{n}.npy") for n in ("sizes", "stream_checksums", "stream_sample", "stream_sample_positions")}
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        dumps.append(got)
    o = orc.oracle()
    want = [o.encode(synth.g_struct(64, 48, 7654321 + k), 75.0, orc.YUV_420) for k in range(3)]
    assert dumps[0]["sizes"].tolist() == [len(c) for c in want]
    for k, c in enumerate(want):
        b = np.frombuffer(c, np.uint8).astype(np.int64)
        assert dumps[0]["stream_checksums"][k] == float(np.dot(b, np.arange(len(b)) % 65521 + 1))
        pos = dumps[0]["stream_sample_positions"].astype(np.int64)
        inside = pos < len(c)
        assert (dumps[0]["stream_sample"][k][inside] == b[pos[inside]]).all() and (dumps[0]["stream_sample"][k][~inside] == -1).all()
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n


# ---- one frame over several ranks: exchange of band bit strings -------------

def _unstuffed_bits(oracle, img, quality, mode):
    """Entropy-coded segment of the oracle JPEG as a bit array (0xFF00 un-stuffed, padding kept)."""
    from oracle import orc  # noqa: F401
    q = oracle.quality_matrices(quality)
    seg = oracle.scan_bits(img, q, yuv_mode=mode)
    raw = bytes(seg).replace(b"\xff\x00", b"\xff")
    return np.unpackbits(np.frombuffer(raw, np.uint8)), bytes(seg)


def _pack_words(bits):
    """bit array -> MSB-first int32 words (zero padded)"""
    n = (len(bits) + 31) // 32 * 32
    b = np.zeros(n, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b).view(">u4").astype(np.uint32).view(np.int32)


def _host_stitch(words, nbits):
    """What sjpeg_hip_stitch_bands does, in numpy: concatenate at bit granularity, pad with 1-bits,
    stuff 0xFF bytes."""
    bits = []
    for w, n in zip(words, nbits):
        u = np.unpackbits(np.asarray(w, np.int32).view(np.uint32).astype(">u4").view(np.uint8))
        bits.append(u[:int(n)])
    allb = np.concatenate(bits) if bits else np.zeros(0, np.uint8)
    pad = (-len(allb)) % 8
    allb = np.concatenate([allb, np.ones(pad, np.uint8)])
    return np.packbits(allb).tobytes().replace(b"\xff", b"\xff\x00")


def _band_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import orc, synth
    from sjpeg_amd.dist import gather_bands
    o = orc.oracle()
    img = synth.g_struct(200, 120, 31)
    bits, seg = _unstuffed_bits(o, img, 80.0, 1)
    # the true bit length is unknown to the test (padding): drop the final byte's worth, the root
    # re-pads; cut the rest at two arbitrary bit positions -> three "bands", rank 1 holds two of them
    total = len(bits) - 8
    cuts = [0, total // 3 + 5, total // 3 + 5, total] if world == 2 else [0, total]
    lo, hi = (cuts[0], cuts[1]) if rank == 0 else (cuts[2], cuts[3])
    mine = bits[lo:hi]
    words = torch.from_numpy(_pack_words(mine).copy())
    nb = torch.tensor([len(mine)], dtype=torch.int64)
    stride = (total + 31) // 32 + 7
    allw, alln = gather_bands(words, nb, stride, dst=0)
    if rank == 0:
        got = _host_stitch(allw.numpy(), alln.numpy())
        # all but the tail of the stream must match what the oracle wrote
        q.put(allw.shape == (world, stride) and alln.tolist() == [cuts[1] - cuts[0], cuts[3] - cuts[2]]
              and seg.startswith(got[:-2]) and len(got) >= len(seg) - 2)
    else:
        assert allw is None and alln is None
    dist.barrier()
    dist.destroy_process_group()


def test_band_ranges():
    from sjpeg_amd.dist import band_ranges
    assert band_ranges(791, 8)[0] == (0, 98) and band_ranges(791, 8)[-1][1] == 791
    r = band_ranges(10, 4)
    assert [b for b, _ in r][1:] == [e for _, e in r][:-1] and r[0][0] == 0 and r[-1][1] == 10
    assert sum(e > b for b, e in band_ranges(3, 8)) == 3           # fewer segments than ranks


def test_gather_bands_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_band_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok


def test_sink_streams_local_brings_a_rank_its_own_frames():
    """The non-rooted end of the batch path: a rank's packed block to its own host buffer, the offsets read once."""
    import pytest
    import sjpeg_amd as sj
    from sjpeg_amd.dist import sink_streams_local
    rng = np.random.RandomState(3)
    frames = [rng.randint(0, 256, n).astype(np.uint8) for n in (40, 1, 33, 160)]
    out = torch.zeros((4, 176), dtype=torch.uint8)
    sizes = torch.tensor([len(f) for f in frames], dtype=torch.int64)
    for i, f in enumerate(frames):
        out[i, :len(f)] = torch.from_numpy(f)
    packed, offs = _compact_torch(out, sizes, 4, 4 * 176)
    host = torch.zeros(1024, dtype=torch.uint8)
    total, ho = sink_streams_local(packed, offs, 4, host)
    assert total == int(offs[4]) == 48 + 16 + 48 + 160
    for i, f in enumerate(frames):
        assert host[int(ho[i]):int(ho[i]) + len(f)].numpy().tobytes() == f.tobytes()
    with pytest.raises(sj.SjpegError):
        sink_streams_local(packed, offs, 4, torch.zeros(64, dtype=torch.uint8))
