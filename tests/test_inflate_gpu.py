"""The device inflater (csrc/inflate.hip) on the GPU.  Every stream of tests/inflate_cases.py through the raw C ABI, source,
output, status, end bits and workspace inside guard bands: the output equals zlib's, the end bit and the chunk table (starts
and live flags of all chunks, lengths and offsets of the live ones - a dead chunk's are wasted work) EQUAL the restatement's
(tests/inflate_ref.py), read from the debug view of the workspace, and a second run gives the same bytes.  One call with many
streams, corrupt ones among them; the encoder's streams back through the decoder; gzip files; and
`DeviceDataLoader(inflate="device")` against `inflate="zlib"`.  Corrupt streams are the decoder's specified input: they end
with a status."""
import ctypes as C
import gzip
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import data_support  # noqa: E402
import inflate_cases as cases  # noqa: E402
import inflate_ref as ref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B
BY_NAME = {name: (stream, payload) for name, stream, payload in cases.CASES}
# the cases that are also decoded at the other chunk sizes: many short chunks, markers over several of them, a dead chunk
SMALL_CHUNK_CASES = ("smooth64k-mem1", "window_spanning", "false_start", "zeros_then_smooth-device_encoder") + cases.TOKEN_SMALL_CHUNK_CASES


@pytest.fixture(scope="module")
def restated():
    """(name, chunk_bytes) -> the restatement's Result; computed once, shared, never modified"""
    out = {(name, cases.GPU_CHUNK): ref.inflate(stream, len(payload), cases.GPU_CHUNK) for name, stream, payload in cases.CASES}
    for name in SMALL_CHUNK_CASES:
        for chunk in (256, 4096):
            out[(name, chunk)] = ref.inflate(BY_NAME[name][0], len(BY_NAME[name][1]), chunk)
    return out


def guarded_inflate(device, streams, sizes, chunk, what):
    """one acimg_inflate call with every operand in a guard arena -> (outputs as bytes, statuses, end bits, chunk table)"""
    from acimg import _lib, inflate, ops
    L = _lib.load()
    lengths = [len(s) for s in streams]
    total_src, total_out, count = sum(lengths), sum(sizes), len(streams)
    ws_bytes = L.acimg_inflate_workspace(total_src, total_out, count, chunk)
    assert ws_bytes > 0
    arena = GuardArena.for_sizes(device, [total_src, total_out, 4 * count, 8 * count, ws_bytes])
    src = arena.region(total_src, name="src")
    out = arena.region(total_out, fill=SENT, name="out")
    status = arena.region(4 * count, fill=SENT, name="status")
    end = arena.region(8 * count, fill=SENT, name="end_bits")
    ws = arena.region(ws_bytes, fill=SENT, name="ws")          # exactly the query's size
    src.u8.copy_(torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()))
    _lib.check(L.acimg_inflate(src.ptr, (C.c_long * count)(*lengths), (C.c_long * count)(*sizes), count, chunk, out.ptr,
                               status.ptr, end.ptr, ws.ptr, ws_bytes, ops.current_stream_handle(device)), what)
    torch.cuda.synchronize(device)
    arena.check(what)
    host = out.u8.cpu().numpy()
    ends = np.cumsum(sizes)
    nchunks = sum(-(-n // chunk) for n in lengths)
    table = ws.u8[:nchunks * inflate.CHUNK_DTYPE.itemsize].cpu().numpy().view(inflate.CHUNK_DTYPE)
    return ([host[e - k:e].tobytes() for e, k in zip(ends, sizes)], status.view(torch.int32, count).cpu().tolist(),
            end.view(torch.int64, count).cpu().tolist(), table)


def same_table(table, r, what):
    """the device's chunk records of one stream against the restatement's"""
    assert table["index"].tolist() == list(range(len(r.starts))), what
    assert table["start"].tolist() == r.starts, (what, "starts")
    assert table["live"].tolist() == r.live, (what, "live")
    live = np.array(r.live, bool)
    assert table["length"][live].tolist() == [n for n, l in zip(r.lengths, r.live) if l], (what, "lengths")
    assert table["offset"][live].tolist() == [o for o, l in zip(r.offsets, r.live) if l], (what, "offsets")


@pytest.mark.parametrize("name", [c[0] for c in cases.CASES])
def test_stream_equals_zlib_and_the_restatement_and_repeats(device, restated, name):
    stream, payload = BY_NAME[name]
    chunks = (cases.GPU_CHUNK,) + ((256, 4096) if name in SMALL_CHUNK_CASES else ())
    for chunk in chunks:
        what = "%s, chunk_bytes %d" % (name, chunk)
        (got,), (st,), (end,), table = guarded_inflate(device, [stream], [len(payload)], chunk, what)
        r = restated[(name, chunk)]
        assert st == ref.OK == r.status, what
        assert torch.equal(torch.frombuffer(bytearray(got), dtype=torch.uint8),
                           torch.frombuffer(bytearray(zlib.decompress(stream, -15)), dtype=torch.uint8)), what
        assert end == r.end_bits and (end + 7) // 8 == len(stream), what
        same_table(table, r, what)
        (again,), (st2,), (end2,), table2 = guarded_inflate(device, [stream], [len(payload)], chunk, what + " (second run)")
        assert again == got and (st2, end2) == (st, end) and table2.tobytes() == table.tobytes(), what


def test_chunks_decode_side_by_side_on_the_device(device, restated):
    stream, payload = BY_NAME[cases.COVERAGE_CASE]
    _, _, _, table = guarded_inflate(device, [stream], [len(payload)], 1024, "coverage")
    later = table["live"][1:]
    assert len(later) >= 12 and 4 * int(later.sum()) >= 3 * len(later)
    _, _, _, table = guarded_inflate(device, [BY_NAME["false_start"][0]], [len(BY_NAME["false_start"][1])], cases.GPU_CHUNK, "bait")
    assert table["start"][1] == 8 * cases.GPU_CHUNK and table["live"].tolist() == [1] + [0] * (len(table) - 1)


@pytest.mark.parametrize("count", [1, 7, 33])
def test_one_call_with_mixed_streams(device, restated, count):
    """streams of unequal sizes in one call, every third a corrupt one: their status is set (the restatement's), their
    neighbours' bytes are intact, nothing outside the extents is touched (the guard bands; a failed stream's own extent is
    unspecified)"""
    good = [c for c in cases.CASES if len(c[2]) <= 16384 or c[0] == cases.COVERAGE_CASE]
    bad = cases.corrupt_streams()
    picks = []
    for i in range(count):
        if i % 3 == 1:
            name, stream, size, status = bad[(i // 3) % len(bad)]
            picks.append((name, stream, size, status, None))
        else:
            name, stream, payload = good[(5 * i + count) % len(good)]
            picks.append((name, stream, len(payload), ref.OK, payload))
    outs, status, ends, table = guarded_inflate(device, [p[1] for p in picks], [p[2] for p in picks], cases.GPU_CHUNK,
                                                "%d streams" % count)
    at = 0
    for i, ((name, stream, size, want, payload), got, st, end) in enumerate(zip(picks, outs, status, ends)):
        k = -(-len(stream) // cases.GPU_CHUNK)
        rows = table[at:at + k]
        at += k
        assert st == want, (name, st, want)
        assert (rows["stream"] == i).all() and rows["index"].tolist() == list(range(k)), name
        if payload is None:
            assert end == 0, name
            continue
        assert got == payload, name
        r = restated[(name, cases.GPU_CHUNK)]
        assert end == r.end_bits, name
        same_table(rows, r, name)
    assert at == len(table)


def test_corrupt_streams_alone_end_with_their_status(device):
    for name, stream, size, want in cases.corrupt_streams():
        _, (st,), (end,), _ = guarded_inflate(device, [stream], [size], cases.GPU_CHUNK, name)
        assert (st, end) == (want, 0), (name, st, want)
    # truncation at every byte of a short multi-block stream
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    smooth = cases.smooth_ramp(3).tobytes()
    stream = co.compress(smooth) + co.flush()
    cuts = list(range(1, len(stream)))
    _, status, _, _ = guarded_inflate(device, [stream[:n] for n in cuts], [len(smooth)] * len(cuts), 256, "every cut")
    assert status == [ref.TRUNCATED] * len(cuts)


def test_round_trip_through_the_device_encoder(device):
    from acimg.deflate import DeviceDeflater
    from acimg.inflate import DeviceInflater
    rng = np.random.RandomState(4)
    image = cases.smooth_ramp(200).tobytes()                          # 100 KiB: seven encoder blocks
    payloads = [image, bytes(40000), rng.randint(0, 256, 50001).astype(np.uint8).tobytes(), b"\x07", image[:16385]]
    streams = DeviceDeflater(device).compress_many(payloads)
    di = DeviceInflater(device, chunk_bytes=4096)
    outs, status, ends = di.inflate_many(streams, [len(p) for p in payloads])
    assert status == [0] * len(payloads) and [(e + 7) // 8 for e in ends] == [len(s) for s in streams]
    for o, p in zip(outs, payloads):
        assert o.device == device and o.cpu().numpy().tobytes() == p
    assert di.inflate(streams[0], len(image)) == image
    assert int(di.chunk_table(-(-len(streams[0]) // 4096))["live"].sum()) >= 3      # the encoder's blocks are found
    with pytest.raises(ValueError):
        di.inflate(streams[0], len(image) + 1)
    data = zlib.compress(image, 9)
    assert di.zlib(data, len(image)) == image
    with pytest.raises(ValueError):
        di.zlib(data[:-1] + bytes([data[-1] ^ 1]), len(image))


def test_gunzip_many_on_files(device, tmp_path):
    from acimg import tfio
    from acimg.inflate import DeviceInflater
    rng = np.random.RandomState(9)
    records = [cases.smooth_ramp(64).tobytes() + rng.bytes(3000), rng.bytes(5000), b"x" * 70000]
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / ("part%d.tfrecord" % k)))
        tfio.write_tfrecord(paths[-1], records[:k + 1], "GZIP")
    raws = [open(p, "rb").read() for p in paths]
    want = [gzip.decompress(r) for r in raws]
    two = raws[0] + raws[1]                                              # two members: the device path must hand it over
    flipped = bytearray(raws[2])
    flipped[len(flipped) // 2] ^= 0x04
    di = DeviceInflater(device, chunk_bytes=1024)
    got = di.gunzip_many(raws + [two])
    assert [g.tobytes() for g in got] == want + [want[0] + want[1]]
    assert di.gunzip(raws[1]) == want[1]
    assert list(tfio.read_tfrecord(paths[2])) == records
    from acimg import _lib
    with pytest.raises(_lib.AcimgError):
        di.gunzip_many([raws[0], bytes(flipped)])                        # a status or the CRC-32: the host's reader raises
    with pytest.raises(_lib.AcimgError):
        di.gunzip(raws[0][:-9] + raws[0][-8:])


# ---- the loader ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record_files(tmp_path_factory):
    """five GZIP files of one 12-frame record each (4 workers: a group of four and a group of one): smooth video in three of
    them (dynamic blocks), random video in two (stored blocks)"""
    from acimg import tfio
    tmp = tmp_path_factory.mktemp("inflate_records")
    rng = np.random.RandomState(17)
    y, x = np.mgrid[0:224, 0:298]
    paths = []
    for r in range(5):
        ai, sa, vi = data_support.outdoor_arrays(rng, wide=True)
        if r % 2 == 0:
            vi = np.stack([np.stack([(127.5 + 100 * np.sin(x / (40.0 + 9 * c) + f) * np.cos(y / (55.0 + 7 * f) + r))
                                     for c in range(3)], -1) for f in range(12)]).astype(np.uint8)
        p = str(tmp / ("part%d.tfrecord" % r))
        tfio.write_tfrecord(p, [data_support.outdoor_example(ai, sa, vi, 2 + r, 7 + 3 * r)], compression="GZIP")
        paths.append(p)
    return paths


@pytest.mark.parametrize("bs", [5, 64])
def test_loader_with_device_inflate_equals_zlib(device, record_files, bs):
    from acimg.data import DeviceDataLoader
    for workers in (1, 4):
        passes = {}
        for mode in ("zlib", "device"):
            dl = DeviceDataLoader(record_files, bs, shuffle=True, buffer_size=24, seed=3, workers=workers, device=device,
                                  inflate=mode)
            passes[mode] = [tuple(t.cpu() for t in b) for b in dl.data]
            assert ("inflate_device" in dl.times) == (mode == "device")
            if mode == "device":
                assert dl.times["inflate_device"] > 0
            dl.close()
        assert len(passes["device"]) == len(passes["zlib"]) == -(-60 // bs)
        for k, (g, w) in enumerate(zip(passes["device"], passes["zlib"])):
            assert len(g) == len(w) == 6
            for a, b in zip(g, w):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (bs, workers, k)


def test_loader_raises_on_a_corrupt_file_either_way(device, record_files, tmp_path):
    from acimg.data import DeviceDataLoader
    raw = bytearray(open(record_files[0], "rb").read())
    raw[len(raw) // 2] ^= 0x20
    bad = str(tmp_path / "bad.tfrecord")
    with open(bad, "wb") as f:
        f.write(bytes(raw))
    for mode in ("zlib", "device"):
        dl = DeviceDataLoader([record_files[1], bad], 8, workers=2, device=device, inflate=mode)
        with pytest.raises((RuntimeError, IOError, ValueError)):
            for _ in dl.data:
                pass
        dl.close()
