"""The device DEFLATE encoder (acimg.deflate) on one GPU against the host's zlib on one thread, on the three payloads the
tools compress, and the two converters end to end with each value of their --deflate switch:

* per payload - a 12-frame record of `acimg.convert` (framed, 2.4 MB of video_like frames), a 464 KB box record of
  `acimg.convert_boxes`, the PNG rows of one 224 x 298 overlay frame: MB/s of input and output / input
  - of the three launches of `acimg_deflate` alone, the payload on the device (device events over --launches calls; the
    call waits for its block table once, so this is the time of a call, not of kernels in a queue),
  - of `DeviceDeflater.deflate` as the tools call it (host bytes in, host bytes out: upload, call, two downloads),
  - of `zlib.compress` at levels 1, 6 and 9,
  and the milliseconds of `zlib.crc32` / `zlib.adler32` over the payload, which stay on the host.
* per block: the time of a ONE-block launch on zeros (a walk of 65 steps), on the smooth fixture's first block and on
  noise (a walk of 16384 steps, every position a literal): the difference is what the one-lane greedy walk costs; and of
  `acimg_huffman_lengths` on one 286-symbol histogram (the code construction's one-thread part dominates it).
* end to end: `acimg.convert.convert` on --seconds records and `acimg.convert_boxes.convert` on --files files, --repeats
  times each with `deflate="device"` and `deflate="zlib"` ALTERNATELY after one warm-up pass of each; records (files)
  per second of wall time and deflate's share of the summed seconds.
* `--assemble host|device|both` (default host: nothing more is run): ONE `acimg_checksum` over 8 device-resident records per
  kind (device events over --launches calls; a call waits for its tables once) beside `zlib.crc32`, `acimg_crc32c` and
  `zlib.adler32` over the same bytes on one host thread; one `acimg_record_gather` of those 8 records; and
  `acimg.convert.convert` with `deflate="device"` and the chosen value(s) of `assemble`, for `both` ALTERNATELY after one
  warm-up pass of each: records per second (min - max over --repeats) and the split of `Converter.times`.
  `--skip_payloads` leaves out the per-payload and per-block parts.
Prints one JSON line.

    python tools/bench_deflate.py --seconds 10 --files 64 --workers 4 --repeats 3
    python tools/bench_deflate.py --seconds 10 --workers 4 --repeats 3 --assemble both --skip_payloads --no_convert
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def host_seconds(call, repeats):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


class RawCall(object):
    """`acimg_deflate` on one payload that already lies on the device"""

    def __init__(self, dev, payload):
        from acimg import _lib, ops
        self.L, self.dev, self.n = _lib.load(), dev, len(payload)
        self.src = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
        self.out_bytes = self.L.acimg_deflate_bound(self.n)
        self.ws_bytes = self.L.acimg_deflate_workspace(self.n, 1)
        self.out = torch.empty(self.out_bytes, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.sizes = torch.empty(1, dtype=torch.int64, device=dev)
        self.lengths = (C.c_long * 1)(self.n)
        self.stream = ops.current_stream_handle(dev)

    def __call__(self):
        from acimg import _lib
        _lib.check(self.L.acimg_deflate(self.src.data_ptr(), self.lengths, 1, self.out.data_ptr(), self.out_bytes,
                                        self.sizes.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self.stream), "deflate")

    def seconds(self, launches, repeats):
        for _ in range(3):
            self()
        out = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(self.dev)
            e0.record()
            for _ in range(launches):
                self()
            e1.record()
            torch.cuda.synchronize(self.dev)
            out.append(e0.elapsed_time(e1) * 1e-3 / launches)
        return out


def event_seconds(dev, call, launches, repeats):
    for _ in range(3):
        call()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) * 1e-3 / launches)
    return out


def checksum_part(dev, record, a):
    """one acimg_checksum over 8 copies of `record` on the device, per kind, and the host's checksums of the same bytes"""
    from acimg import _lib, checksum, tfio
    count = 8
    data = torch.from_numpy(np.frombuffer(record * count, np.uint8).copy()).to(dev)
    lengths = [len(record)] * count
    dc = checksum.DeviceChecksum(dev)
    L = _lib.load()
    host = {0: lambda b: zlib.crc32(b), 1: lambda b: L.acimg_crc32c(b, len(b), 0), 2: lambda b: tfio.mask_crc(L.acimg_crc32c(b, len(b), 0)),
            3: lambda b: zlib.adler32(b)}
    out = dict(records=count, bytes_each=len(record))
    for kind, name in ((0, "crc32"), (1, "crc32c"), (2, "crc32c_masked"), (3, "adler32")):
        got = dc.values(dc.packed(data, lengths, kind))
        assert got == [host[kind](record) & 0xFFFFFFFF] * count, name
        dev_s = event_seconds(dev, lambda: dc.packed(data, lengths, kind), a.launches, a.repeats)
        host_s = host_seconds(lambda: [host[kind](record) for _ in range(count)], a.repeats)
        out[name] = dict(device_call_us=spread([t * 1e6 for t in dev_s]), host_one_thread_us=spread([t * 1e6 for t in host_s]))
    # the gather of the same 8 records: 13 skeleton pieces and 12 frames each, frames at the offsets they have in a record
    from acimg import convert
    lay = convert.build_record_layout(convert.Recording("", 1, 1, 1, "", ""), np.zeros((12, 1024), np.int32), 224 * 298 * 3,
                                      (12, 224, 298, 3))
    assert len(lay.skeleton) == len(record)
    pool = torch.zeros(count, 12 * 224 * 298 * 3, dtype=torch.uint8, device=dev)
    skel = torch.from_numpy(np.frombuffer(lay.skeleton * count, np.uint8).copy()).to(dev)
    rows, base = [], 0
    for r in range(count):
        rows += [(base + o, base + o, n, 0) for o, n in lay.pieces()]
        rows += [(base + o, r * pool.shape[1] + j * n, n, 1) for j, (o, n) in enumerate(lay.holes)]
        base += len(lay.skeleton)
    dst = torch.empty(base, dtype=torch.uint8, device=dev)
    t = event_seconds(dev, lambda: dc.gather(skel, pool.view(-1), rows, dst), a.launches, a.repeats)
    out["record_gather"] = dict(segments=len(rows), device_call_us=spread([x * 1e6 for x in t]))
    return out


def payloads(rng, dev):
    import bench_convert
    import bench_convert_boxes

    from acimg import convert, convert_boxes, tfio
    resizer = convert.FrameResizer(dev, bench_convert.H, bench_convert.W)
    frames = resizer.resize_frames(bench_convert.video_like(rng, 12)).cpu().numpy()
    audio = rng.randint(-2 ** 15, 2 ** 15, size=(12, 1024)).astype(np.int32)
    rec = convert.Recording("", 1, 1, 1, "", "")
    record = tfio.frame_record(convert.build_record(rec, audio, frames))
    side = bench_convert_boxes.SIDE
    resizer = convert.FrameResizer(dev, side, side, new_size=(224, 298))
    video = resizer.resize_frames(bench_convert_boxes.photo_like(rng, 1)).cpu().numpy()[0]
    t = np.arange(66000)
    clip = (2 ** 13 * np.sin(2 * np.pi * 700.0 * t / 12288.0) + rng.randn(t.size) * 300).astype(np.int32)
    boxes = [[40, 0, 0], [200, 0, 0], [50, 0, 0], [220, 0, 0]]
    box = tfio.frame_record(convert_boxes.build_box_record(boxes, [1, 0, 0], clip, video))
    grey = frames[0].mean(2, keepdims=True).astype(np.uint8).repeat(3, 2)        # an overlay is a grey frame under a colour map
    rows = np.zeros((224, 1 + 3 * 298), np.uint8)
    rows[:, 1:] = grey.reshape(224, -1)
    return (("convert_record_12_frames", record), ("box_record", box), ("png_rows_224x298", rows.tobytes()))


def assemble_part(dev, rng, a):
    """acimg.convert.convert with deflate="device" and each chosen value of `assemble`, alternately"""
    import bench_convert

    from acimg import convert
    modes = ("host", "device") if a.assemble == "both" else (a.assemble,)
    tmp = tempfile.mkdtemp(prefix="bench_assemble_", dir=a.tmp)
    try:
        raw, outd = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        bench_convert.write_tree(raw, rng, a.seconds)
        rates, times, digest = {m: [] for m in modes}, {m: [] for m in modes}, {}
        for rep in range(a.repeats + 1):              # the first pass of each is the warm-up
            for mode in modes:
                shutil.rmtree(outd, ignore_errors=True)
                os.makedirs(outd)
                t0 = time.perf_counter()
                paths, conv = convert.convert(raw, outd, device=str(dev), workers=a.workers, deflate="device", assemble=mode)
                dt = time.perf_counter() - t0
                digest[mode] = [zlib.crc32(open(p, "rb").read()) for p in paths]
                if rep:
                    rates[mode].append(len(paths) / dt)
                    times[mode].append(dict(conv.times))
        out = {m: dict(per_s=spread(rates[m]),
                       times_s={k: statistics.median(t[k] for t in times[m]) for k in ("read", "device", "deflate")},
                       deflate_share=statistics.median(t["deflate"] / sum(t.values()) for t in times[m])) for m in modes}
        out.update(workers=a.workers, records=a.seconds)
        if len(modes) == 2:
            out["same_files"] = digest["host"] == digest["device"]
            out["slowest_device_above_fastest_host"] = out["device"]["per_s"]["min"] > out["host"]["per_s"]["max"]
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--tmp", type=str, default=None)
    ap.add_argument("--no_convert", action="store_true", help="the payloads and the blocks alone (a kernel-trace run)")
    ap.add_argument("--assemble", default="host", choices=("host", "device", "both"),
                    help="device / both: time acimg_checksum and the converter with --assemble device (both: against host)")
    ap.add_argument("--skip_payloads", action="store_true", help="leave out the per-payload and per-block parts")
    a = ap.parse_args()
    import bench_convert
    import bench_convert_boxes
    import deflate_cases

    from acimg import _lib, convert, convert_boxes, jpeg, ops
    from acimg.deflate import BLOCK, DeviceDeflater

    dev = torch.device("cuda:0")
    L = _lib.load()
    rng = np.random.RandomState(0)
    dd = DeviceDeflater(dev)
    res = dict(block=BLOCK, repeats=a.repeats, launches=a.launches)

    # ---- the payloads ---------------------------------------------------------------------------------------------------------
    named = payloads(rng, dev)
    for name, p in ([] if a.skip_payloads else named):
        mb = len(p) * 1e-6
        stream = dd.deflate(p)
        assert zlib.decompress(stream, -15) == p, name
        one = dict(bytes=len(p), device_ratio=len(stream) / len(p))
        one["device_call_mb_per_s"] = spread([mb / t for t in RawCall(dev, p).seconds(a.launches, a.repeats)])
        one["device_host_to_host_mb_per_s"] = spread([mb / t for t in host_seconds(lambda: dd.deflate(p), a.repeats)])
        for level in (1, 6, 9):
            t = host_seconds(lambda: zlib.compress(p, level), a.repeats)
            one["zlib_%d" % level] = dict(ratio=(len(zlib.compress(p, level)) - 6) / len(p), mb_per_s=spread([mb / x for x in t]))
        one["crc32_ms"] = min(host_seconds(lambda: zlib.crc32(p), a.repeats)) * 1e3
        one["adler32_ms"] = min(host_seconds(lambda: zlib.adler32(p), a.repeats)) * 1e3
        res[name] = one

    if a.assemble != "host":
        res["checksum_8_records"] = checksum_part(dev, named[0][1], a)
        res["assemble"] = assemble_part(dev, rng, a)
    if a.skip_payloads:
        print(json.dumps(res))
        return

    # ---- one block ------------------------------------------------------------------------------------------------------------
    blocks = dict(zeros=bytes(BLOCK), smooth=deflate_cases.smooth_fixture()[:BLOCK],
                  noise=rng.randint(0, 256, BLOCK).astype(np.uint8).tobytes())
    res["one_block_us"] = {k: spread([t * 1e6 for t in RawCall(dev, p).seconds(a.launches, a.repeats)])
                           for k, p in blocks.items()}
    freq = torch.from_numpy(rng.randint(1, 4000, size=(1, 286)).astype(np.int32)).to(dev)
    lens = torch.empty(1, 286, dtype=torch.uint8, device=dev)
    st = ops.current_stream_handle(dev)

    def code():
        _lib.check(L.acimg_huffman_lengths(freq.data_ptr(), 1, 286, 15, lens.data_ptr(), st), "huffman_lengths")
    for _ in range(3):
        code()
    t = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.launches):
            code()
        e1.record()
        torch.cuda.synchronize(dev)
        t.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    res["huffman_lengths_286_us"] = spread(t)

    # ---- the converters, the two switch values alternately ---------------------------------------------------------------------
    if not a.no_convert:
        tmp = tempfile.mkdtemp(prefix="bench_deflate_", dir=a.tmp)
        try:
            raw_a, raw_b, outd = os.path.join(tmp, "raw_a"), os.path.join(tmp, "raw_b"), os.path.join(tmp, "out")
            bench_convert.write_tree(raw_a, rng, a.seconds)
            photos = torch.from_numpy(bench_convert_boxes.photo_like(rng, a.files))
            jpegs = jpeg.JpegEncoder(dev, 90, restart_mcus=256).encode(photos)
            rate = 44100
            bench_convert_boxes.write_tree(raw_b, jpegs, (rng.randn(rate * 10) * 3000).astype(np.int32), rate)
            runs = (("convert", lambda mode: convert.convert(raw_a, outd, device=str(dev), workers=a.workers, deflate=mode)),
                    ("convert_boxes", lambda mode: convert_boxes.convert(raw_b, outd, device=str(dev), workers=a.workers,
                                                                         list_file=os.path.join(tmp, "list.txt"), deflate=mode)))
            for name, run in runs:
                rates, shares, sizes = dict(device=[], zlib=[]), dict(device=[], zlib=[]), {}
                for rep in range(a.repeats + 1):          # the first pass of each is the warm-up
                    for mode in ("device", "zlib"):
                        shutil.rmtree(outd, ignore_errors=True)
                        os.makedirs(outd)
                        t0 = time.perf_counter()
                        paths, conv = run(mode)
                        dt = time.perf_counter() - t0
                        sizes[mode] = os.path.getsize(paths[0])
                        if rep:
                            rates[mode].append(len(paths) / dt)
                            shares[mode].append(conv.times["deflate"] / sum(conv.times.values()))
                res[name] = {mode: dict(per_s=spread(rates[mode]), deflate_share=statistics.median(shares[mode]),
                                        record_file_bytes=sizes[mode]) for mode in ("device", "zlib")}
                res[name]["workers"] = a.workers
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
