"""The device DEFLATE encoder (csrc/deflate.hip) on the GPU.  Every payload of tests/deflate_cases.py through the raw C ABI,
input, output, sizes and workspace inside guard bands: the stream inflates to the payload with zlib, equals the
restatement (tests/deflate_ref.py) byte for byte, is the same on a second run and stays within acimg_deflate_bound.
Two calls with more blocks than the offsets kernel has threads.  `acimg_huffman_lengths` on the CPU test's histograms;
`compress_many`; and the three tools' smallest inputs end to end:
records written with `--deflate device` read by the project's loaders, a PNG written with the device deflater."""
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

import convert_boxes_support as support  # noqa: E402
import convert_ref  # noqa: E402
import deflate_cases as cases  # noqa: E402
import deflate_ref as ref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B


@pytest.fixture(scope="module")
def restated():
    """name -> the restatement's stream; computed once, shared"""
    return {name: ref.deflate(p) for name, p in cases.PAYLOADS}


def guarded_deflate(device, payloads, what):
    """one acimg_deflate call on `payloads` with every operand in a guard arena -> their streams"""
    from acimg import _lib, ops
    L = _lib.load()
    lengths = [len(p) for p in payloads]
    total, count = sum(lengths), len(payloads)
    out_bytes = sum(L.acimg_deflate_bound(n) for n in lengths)
    ws_bytes = L.acimg_deflate_workspace(total, count)
    arena = GuardArena.for_sizes(device, [total, out_bytes, 8 * count, ws_bytes])
    src = arena.region(total, name="in")
    out = arena.region(out_bytes, fill=SENT, name="out")
    sizes = arena.region(8 * count, fill=SENT, name="out_sizes")
    ws = arena.region(ws_bytes, fill=SENT, name="ws")
    src.u8.copy_(torch.from_numpy(np.frombuffer(b"".join(payloads), np.uint8).copy()))
    _lib.check(L.acimg_deflate(src.ptr, (C.c_long * count)(*lengths), count, out.ptr, out_bytes, sizes.ptr, ws.ptr, ws_bytes,
                               ops.current_stream_handle(device)), what)
    torch.cuda.synchronize(device)
    arena.check(what)
    n = sizes.view(torch.int64, count).cpu().tolist()
    host = out.u8.cpu().numpy()
    assert all(0 < k <= L.acimg_deflate_bound(m) for k, m in zip(n, lengths)), (what, n)
    assert (host[sum(n):] == SENT).all(), "%s: bytes behind the streams were written" % what
    ends = np.cumsum(n)
    return [host[e - k:e].tobytes() for e, k in zip(ends, n)]


@pytest.mark.parametrize("name,payload", cases.PAYLOADS, ids=[n for n, _ in cases.PAYLOADS])
def test_stream_inflates_equals_the_restatement_and_repeats(device, restated, name, payload):
    (got,) = guarded_deflate(device, [payload], name)
    assert zlib.decompress(got, -15) == payload
    assert len(got) <= ref.bound(len(payload))
    assert got == restated[name], "%s: %d bytes, the restatement has %d" % (name, len(got), len(restated[name]))
    (again,) = guarded_deflate(device, [payload], name + " (second run)")
    assert again == got


def test_more_blocks_than_the_offsets_kernel_has_threads(device):
    """deflate_offsets_kernel gives each of its 1024 threads ceil(nblocks / 1024) consecutive blocks: 1025 blocks are the
    first call in which a thread holds two, and in the call of 2053 three payloads lie across two threads' blocks, the
    last one among them, so that a payload's first block is summed by another thread than its last.  Every stream and
    every entry of out_sizes against the restatement, inside guard bands."""
    for name, payloads in cases.many_block_calls():
        nblocks, per_thread, runs = cases.block_runs(payloads)
        across = [r for r in runs if r[0] // per_thread != r[1] // per_thread]
        if name == "1025_of_one_byte":
            assert (nblocks, per_thread) == (1025, 2)
        else:
            assert nblocks >= 2049 and per_thread >= 3 and len(across) >= 2 and runs[-1] in across
        got = guarded_deflate(device, payloads, name)
        assert len(got) == len(payloads)
        memo = {}
        for i, (p, g) in enumerate(zip(payloads, got)):
            if p not in memo:
                memo[p] = ref.deflate(p)
            assert g == memo[p], "%s: payload %d of %d bytes (blocks %d..%d)" % (name, i, len(p), runs[i][0], runs[i][1])


def test_matching_is_alive(device):
    """the smooth fixture must come out smaller than zlib's Z_HUFFMAN_ONLY over the same 32 KiB chunks (176 030 bytes;
    chunked level 1 reaches 105 576): a condition a broken matcher cannot meet, no tuning target.  Noise stays in bound."""
    from acimg.deflate import DeviceDeflater
    payload = cases.smooth_fixture()
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    huffman_only = 0
    for s in range(0, len(payload), 32768):
        huffman_only += len(co.compress(payload[s:s + 32768])) + len(co.flush(zlib.Z_FULL_FLUSH))
    huffman_only += len(co.flush())
    dd = DeviceDeflater(device)
    got = dd.deflate(payload)
    print("smooth fixture: device %d bytes, zlib Z_HUFFMAN_ONLY chunked %d" % (len(got), huffman_only))
    assert zlib.decompress(got, -15) == payload
    assert len(got) < min(huffman_only, 176030)
    noise = dict(cases.PAYLOADS)["noise_%d" % (3 * ref.BLOCK + 17)]
    assert len(noise) < len(dd.deflate(noise)) <= ref.bound(len(noise))


@pytest.mark.parametrize("nsym,limit", cases.ALPHABETS)
def test_huffman_lengths_equal_the_restatement(device, nsym, limit):
    from acimg import _lib, ops
    L = _lib.load()
    rows = cases.histogram_rows(nsym)
    rows[-1, 0] = -4                                     # a negative count is an unused symbol
    n = rows.shape[0]
    arena = GuardArena.for_sizes(device, [rows.nbytes, n * nsym])
    freq = arena.region(rows.nbytes, name="freq")
    out = arena.region(n * nsym, fill=SENT, name="lengths")
    freq.view(torch.int32, n, nsym).copy_(torch.from_numpy(rows))
    _lib.check(L.acimg_huffman_lengths(freq.ptr, n, nsym, limit, out.ptr, ops.current_stream_handle(device)), "huffman_lengths")
    torch.cuda.synchronize(device)
    arena.check("huffman_lengths")
    got = out.view(torch.uint8, n, nsym).cpu().numpy()
    for r in range(n):
        assert got[r].tolist() == ref.huffman_lengths(rows[r], limit), "row %d" % r
        cases.check_lengths(np.maximum(rows[r], 0), got[r], limit, "row %d" % r)


def test_compress_many(device, restated):
    from acimg.deflate import DeviceDeflater
    by_name = dict(cases.PAYLOADS)
    names = ["period4", "one_literal_twice", None, "fibonacci_counts", "noise_%d" % (ref.BLOCK + 1)]
    payloads = [b"" if k is None else by_name[k] for k in names]
    want = [ref.EMPTY_FINAL if k is None else restated[k] for k in names]
    dd = DeviceDeflater(device)
    assert dd.compress_many(payloads) == want
    assert dd.compress_many([]) == [] and dd.compress_many([b"", b""]) == [ref.EMPTY_FINAL] * 2
    # the same through the raw ABI inside guard bands: no stream disturbs its neighbour
    assert guarded_deflate(device, [p for p in payloads if p], "four payloads") == [w for k, w in zip(names, want) if k]
    # tensors on the device and containers
    t = torch.from_numpy(np.frombuffer(payloads[3], np.uint8).copy()).to(device)
    assert dd.deflate(t) == want[3]
    assert gzip.decompress(dd.gzip(payloads[0])) == payloads[0] and zlib.decompress(dd.zlib(payloads[3])) == payloads[3]
    assert gzip.decompress(dd.gzip(b"")) == b"" and zlib.decompress(dd.zlib(b"")) == b""


# ---- end to end, at the tools' smallest inputs --------------------------------------------------------------------------------
def test_convert_with_device_deflate_is_read_by_the_loader(device, tmp_path):
    from acimg import convert, tfio
    from acimg.data import TFRecordDataLoader
    rng = np.random.RandomState(13)
    raw = tmp_path / "raw"
    raw.mkdir()
    ramp = (np.arange(480)[:, None, None] // 2 + np.arange(640)[None, :, None] // 4 + np.arange(3)[None, None, :] * 9) % 256
    frames = (ramp[None] + rng.randint(0, 3, size=(12, 480, 640, 3))).astype(np.uint8)     # smooth: dynamic blocks
    sound = rng.randint(-2 ** 15, 2 ** 15, size=12288 + 5)
    convert_ref.write_recording(raw, 2, 4, 1, frames, sound)
    got = {}
    for mode in ("zlib", "device"):
        out = tmp_path / mode
        out.mkdir()
        lst = str(out / "list.txt")
        assert convert.main([str(raw), str(out), "--list", lst, "--device", str(device), "--workers", "2", "--deflate", mode]) == 0
        (path,) = open(lst).read().split()
        with open(path, "rb") as f:
            data = f.read()
        assert data[:2] == b"\x1f\x8b"
        (batch,) = list(TFRecordDataLoader(lst, 12, device=device, modalities=(1, 2)).data)    # the native zlib reader
        got[mode] = (data, list(tfio.read_tfrecord(path)), [t.cpu() for t in batch if isinstance(t, torch.Tensor)])
    assert got["device"][1] == got["zlib"][1]
    assert len(got["device"][2]) == len(got["zlib"][2]) >= 5
    for a, b in zip(got["device"][2], got["zlib"][2]):
        assert torch.equal(a, b)
    framed = gzip.decompress(got["device"][0])
    assert got["device"][0][10:-8] == ref.deflate(framed) and len(got["device"][0]) < len(framed)


def test_convert_boxes_with_device_deflate_is_read_by_the_loader(device, tmp_path):
    from acimg import convert_boxes as cb
    from acimg.data import BoxRecordLoader
    with np.load(cases.GOLDEN) as g:
        jpg = g["jpeg_smooth_420_256x256"].tobytes()
    raw = tmp_path / "raw"
    (raw / "Dataset" / "Annotations").mkdir(parents=True)
    (raw / "Dataset" / "Data" / "0").mkdir(parents=True)
    wave = (2 ** 13 * np.sin(2 * np.pi * 700.0 * np.arange(1500) / 12288.0)).astype(np.int32)
    (raw / "Dataset" / "Data" / "0" / "1001.jpg").write_bytes(jpg)
    (raw / "Dataset" / "Data" / "0" / "1001.wav").write_bytes(convert_ref.wav_bytes(wave, rate=12288, bits=16))
    (raw / "Dataset" / "Annotations" / "1001.xml").write_bytes(support.annotation_xml("1001", [("object", 64, 4, 192, 12)]))
    (raw / "test_list.txt").write_text("1001.jpg\n")
    got = {}
    for mode in ("zlib", "device"):
        out = tmp_path / mode
        out.mkdir()
        lst = str(out / "test.txt")
        assert cb.main([str(raw), str(out), "--list", lst, "--device", str(device), "--workers", "2", "--deflate", mode]) == 0
        data = (out / "1001.tfrecord").read_bytes()
        assert data[:2] == b"\x1f\x8b"
        (batch,) = list(BoxRecordLoader(lst, 1))
        got[mode] = (data, [t for t in batch if isinstance(t, torch.Tensor)])
    assert gzip.decompress(got["device"][0]) == gzip.decompress(got["zlib"][0])
    assert len(got["device"][1]) == len(got["zlib"][1]) >= 8
    for a, b in zip(got["device"][1], got["zlib"][1]):
        assert torch.equal(a, b)
    assert got["device"][0][10:-8] == ref.deflate(gzip.decompress(got["zlib"][0]))


def test_png_with_the_device_deflater_decodes_to_the_same_pixels(device, tmp_path):
    from acimg import png
    from acimg.deflate import DeviceDeflater
    rng = np.random.RandomState(8)
    img = ((np.arange(224)[:, None, None] + np.arange(298)[None, :, None] // 2 + np.arange(3) * 40) % 256
           + rng.randint(0, 2, (224, 298, 3))).astype(np.uint8)
    n = png.write_png(str(tmp_path / "frame.png"), img, deflater=DeviceDeflater(device))
    data = (tmp_path / "frame.png").read_bytes()
    assert len(data) == n and data[:8] == png.SIGNATURE and data[12:16] == b"IHDR" and data[37:41] == b"IDAT"
    assert int.from_bytes(data[16:20], "big") == 298 and int.from_bytes(data[20:24], "big") == 224
    k = int.from_bytes(data[33:37], "big")
    assert int.from_bytes(data[41 + k:45 + k], "big") == zlib.crc32(data[37:41 + k]) and data[-8:-4] == b"IEND"
    rows = np.frombuffer(zlib.decompress(data[41:41 + k]), np.uint8).reshape(224, 1 + 3 * 298)     # filter byte 0, then RGB
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(224, 298, 3), img)
    assert k < len(zlib.compress(rows.tobytes(), 0))
