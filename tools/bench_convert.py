"""The dataset converter on one GPU, at the reference's camera geometry (640 x 480 BMP frames -> 224 x 298):

* the kernel alone (`acimg_resize_cubic_u8` on BMP-shaped operands: pixels from byte 54, bottom-up rows) at 12 and 120
  frames per launch: --launches back-to-back launches between two device events, --repeats times after a warm-up;
  frames/s, and GB/s of the bytes the algorithm has to move (every source byte once in, every output byte once out) -
  a rate of bytes moved, not of HBM traffic: the operands of a launch fit the Infinity Cache.  `rows_read_twice` is the
  share of source rows that more than one band of 8 output rows reads (from the tap tables; the L2 serves the second).
* the converter end to end (`acimg.convert.convert`) on a tree of --seconds one-second records written to --tmp: records/s
  of wall time, and where the time goes: `read` and `deflate` are summed over the --workers threads, `device` (upload +
  resize + download) is wall time of the calling thread.  `--deflate device` compresses the records on the GPU
  (acimg.deflate) instead of gzip level 9 on the workers; tools/bench_deflate.py runs both alternately.
* the NumPy restatement (tests/convert_ref.py) of one frame on the host, for scale.
Prints one JSON line.

    python tools/bench_convert.py --seconds 10 --workers 4 --repeats 5
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, OH, OW, BAND = 480, 640, 224, 298, 8


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def video_like(rng, n):
    """frames with the statistics that matter to deflate: smooth structure plus sensor noise"""
    coarse = rng.randint(0, 256, size=(n, H // 8, W // 8, 3)).astype(np.float32)
    smooth = np.kron(coarse, np.ones((1, 8, 8, 1), np.float32))
    return np.clip(smooth + rng.normal(0, 3, size=smooth.shape), 0, 255).astype(np.uint8)


def write_tree(raw, rng, seconds):
    """one recording of `seconds` one-second records under `raw`"""
    import convert_ref as ref
    os.makedirs(raw)
    ref.write_recording(raw, 1, 1, seconds, video_like(rng, 12 * seconds), rng.randint(-2 ** 15, 2 ** 15, size=12288 * seconds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tmp", type=str, default=None)
    ap.add_argument("--deflate", default="zlib", choices=("zlib", "device"))
    a = ap.parse_args()
    import convert_ref as ref

    from acimg import convert

    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    res = dict(height=H, width=W, out_height=OH, out_width=OW, repeats=a.repeats, launches=a.launches)

    # ---- the kernel alone ---------------------------------------------------------------------------------------------------
    rs = convert.FrameResizer(dev, H, W)
    iy = rs.tables[0].cpu().numpy()
    rows = [set(range(int(iy[r0:r0 + BAND].min()), int(iy[r0:r0 + BAND].max()) + 1)) for r0 in range(0, OH, BAND)]
    read, distinct = sum(len(s) for s in rows), len(set().union(*rows))
    res["rows_read_twice"] = (read - distinct) / float(distinct)
    res["source_rows_per_band"] = max(len(s) for s in rows)
    frame = ref.bmp_bytes(video_like(rng, 1)[0])
    lay = convert.parse_bmp_header(frame)
    moved = H * W * 3 + OH * OW * 3
    res["bytes_moved_per_frame"] = moved
    for n in (12, 120):
        src = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).repeat(n, 1).to(dev)
        src += torch.arange(n, dtype=torch.uint8, device=dev)[:, None] * (torch.arange(src.shape[1], device=dev) >= 54)
        out = torch.empty(n, OH, OW, 3, dtype=torch.uint8, device=dev)
        call = lambda: rs.resize(src.reshape(-1), src.shape[1], lay.pixel_offset, lay.row_stride, n, out=out)  # noqa: E731
        for _ in range(20):
            call()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(a.launches):
                call()
            e1.record()
            torch.cuda.synchronize(dev)
            times.append(e0.elapsed_time(e1) * 1e-3 / a.launches)
        res["kernel_%d_frames" % n] = dict(
            us_per_launch=spread([t * 1e6 for t in times]), frames_per_s=spread([n / t for t in times]),
            gb_per_s_moved=spread([n * moved / t * 1e-9 for t in times]))

    # ---- the NumPy restatement, one frame ---------------------------------------------------------------------------------
    one = video_like(rng, 1)[0]
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.convert_frame(one)
        t.append(time.perf_counter() - t0)
    res["numpy_restatement_frames_per_s"] = 1.0 / min(t)

    # ---- end to end -------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="bench_convert_", dir=a.tmp)
    try:
        raw, outd = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        write_tree(raw, rng, a.seconds)
        rates, shares = [], []
        for rep in range(a.repeats + 1):          # the first pass is the warm-up (page cache, code objects)
            shutil.rmtree(outd, ignore_errors=True)
            os.makedirs(outd)
            t0 = time.perf_counter()
            paths, conv = convert.convert(raw, outd, device=str(dev), workers=a.workers, deflate=a.deflate)
            dt = time.perf_counter() - t0
            if rep:
                rates.append(len(paths) / dt)
                tot = sum(conv.times.values())
                shares.append({k: v / tot for k, v in conv.times.items()})
        res["convert"] = dict(records=a.seconds, workers=a.workers, deflate=a.deflate, records_per_s=spread(rates),
                              frames_per_s=spread([12 * r for r in rates]),
                              share={k: statistics.median(s[k] for s in shares) for k in shares[0]},
                              record_file_bytes=os.path.getsize(paths[0]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
