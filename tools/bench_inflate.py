"""The device inflater (acimg.inflate) on one GPU against `zlib.decompress` on one host thread of the same box.

Payloads: the three of tools/bench_deflate.py (a 12-frame record of `acimg.convert`, a box record, the PNG rows of one
overlay frame) and the two records of tools/bench_loader.py (`smooth` and `random` video) - the files the loaders read.
Each is written by zlib at levels 6 and 9 and by the device encoder's restatement-equal streams (`DeviceDeflater`).
Per payload and writer:
  - MB/s of INFLATED bytes of `zlib.decompress(stream, -15)`,
  - MB/s of inflated bytes of the device path, host bytes to host bytes (the streams uploaded, ONE `acimg_inflate` call,
    the output downloaded, the statuses read), at chunk_bytes 16384 / 32768 / 65536 / 131072 and 1, 4 and 16 files per call,
  - the share of the chunks that come out live at each chunk size.
The shipped `acimg.inflate.DEFAULT_CHUNK_BYTES` is the best of the four on the smooth record; 4096 and
8192 are measured beside them for the record.
Prints one JSON line.  --trace: a few calls on the smooth record only (for a `rocprofv3 --kernel-trace --stats` run).

    python tools/bench_inflate.py --repeats 5
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CHUNKS = (16384, 32768, 65536, 131072)      # the candidates for the shipped default
SMALLER = (4096, 8192)                       # measured for the record only
FILES = (1, 4, 16)


def seconds(call, repeats):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def rate(nbytes, secs):
    return dict(median=round(nbytes / statistics.median(secs) / 1e6, 1), min=round(nbytes / max(secs) / 1e6, 1),
                max=round(nbytes / min(secs) / 1e6, 1))


def loader_records():
    """the framed records of one file of tools/bench_loader.py, per content"""
    import bench_loader
    out = []
    with tempfile.TemporaryDirectory(prefix="acimg_inflate_") as tmp:
        for content in ("smooth", "random"):
            path = bench_loader.write_file(os.path.join(tmp, content + ".tfrecord"), content, 1, 3)
            with open(path, "rb") as f:
                out.append(("loader_record_" + content, gzip.decompress(f.read())))
    return out


def device_call(di, streams, sizes, dev):
    out, status, _ = di.inflate_launch(streams, sizes)
    host = out.cpu()
    assert not status.cpu().any()
    return host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="a few calls on the smooth record only")
    a = ap.parse_args()
    from acimg.deflate import DeviceDeflater
    from acimg.inflate import DEFAULT_CHUNK_BYTES, DeviceInflater
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    items = loader_records()
    if a.trace:
        name, payload = items[0]
        stream = zlib.compress(payload, 6)[2:-4]
        di = DeviceInflater(dev)
        for _ in range(5):
            device_call(di, [stream] * 4, [len(payload)] * 4, dev)
        torch.cuda.synchronize(dev)
        print(json.dumps(dict(trace=name, chunk_bytes=DEFAULT_CHUNK_BYTES, files=4, calls=5)))
        return
    import bench_deflate
    items += list(bench_deflate.payloads(rng, dev))
    dd = DeviceDeflater(dev)
    res = dict(repeats=a.repeats, default_chunk_bytes=DEFAULT_CHUNK_BYTES)
    for name, payload in items:
        payload = bytes(payload)
        n = len(payload)
        writers = (("zlib_6", zlib.compress(payload, 6)[2:-4]), ("zlib_9", zlib.compress(payload, 9)[2:-4]),
                   ("device_encoder", dd.deflate(payload)))
        res[name] = dict(bytes=n)
        for wname, stream in writers:
            assert zlib.decompress(stream, -15) == payload
            row = dict(stream_bytes=len(stream), zlib_mb_per_s=rate(n, seconds(lambda: zlib.decompress(stream, -15), a.repeats)))
            for chunk in SMALLER + CHUNKS:
                di = DeviceInflater(dev, chunk_bytes=chunk)
                got = device_call(di, [stream], [n], dev)
                assert got.numpy().tobytes() == payload, (name, wname, chunk)
                table = di.chunk_table(-(-len(stream) // chunk))
                cell = dict(chunks=int(len(table)), live=int(table["live"].sum()))
                for files in FILES:
                    secs = seconds(lambda: device_call(di, [stream] * files, [n] * files, dev), a.repeats)
                    cell["files_%d_mb_per_s" % files] = rate(files * n, secs)
                row["chunk_%d" % chunk] = cell
            res[name][wname] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
