"""The PNG decoder and the two-object test-set converter on one GPU, at the data set's geometry (224 x 298 RGB, 8 bits):

* `acimg_png_unfilter` alone on --files files per launch: every row filter 0, then 1, 2, 3, 4, then a filter drawn per
  row; Adam7 files; and ONE file of 1, 64 and 65 rows at width 298.  --launches back-to-back calls between two device
  events, --repeats times after a warm-up.  `rows64_over_rows1` is the figure that shows the wavefront: 64 rows cost
  298 + 63 steps where one row costs 298, so a ratio near 1 (64 would be a serial walk); a call includes the copy of its
  job table and one wait for the stream, which both sides of the ratio pay.
* `acimg_png_pixels` alone on the same files, plain and Adam7.
* the converter end to end (`acimg.convert_collected.convert`) on a tree of 23 files (the label table holds ids 1 .. 23)
  written to --tmp, with `--inflate` and `--deflate` at both values: files/s of wall time and the `times` split (`read`,
  `parse` and `deflate` summed over the --workers threads, `device` wall time of the calling thread).
* where Pillow is importable, `Image.open(...).load()` of the --files files on 16 host threads, for scale; else it says
  that Pillow was absent.
The pictures are --unique smooth images (tests/png_cases.py `photo`) repeated to --files; the files come from
tests/png_writer.py.  Prints one JSON line.

    python tools/bench_convert_collected.py --files 256 --workers 4 --repeats 5
"""
import argparse
import concurrent.futures
import ctypes as C
import io
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

H, W = 224, 298


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def timed(dev, call, launches, repeats):
    """seconds per launch, `repeats` times"""
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


class Launch(object):
    """the operands of one launch of both kernels for `raws` (inflated streams) of files with `geometry`, on the device"""

    def __init__(self, dev, L, raws, geometry):
        import png_decode_ref as ref
        from acimg import ops
        self.L, self.n, self.st = L, len(raws), ops.current_stream_handle(dev)
        h, w, ct, depth, lace = geometry
        inflated, samples, pixels = ref.sizes(*geometry)
        jobs, files = [], []
        for i in range(self.n):
            jobs += [[i * inflated + s, i * samples + d, rows, rb, bpp, i] for s, d, rows, rb, bpp in ref.job_table(*geometry)]
            files.append([i * samples, h, w, ct, depth, lace, 0, 0, i * pixels])
        self.jobs, self.njobs = (C.c_long * (6 * len(jobs)))(*[v for r in jobs for v in r]), len(jobs)
        self.files = (C.c_long * (9 * self.n))(*[v for r in files for v in r])
        self.src = torch.from_numpy(np.frombuffer(b"".join(raws), np.uint8).copy()).to(dev)
        self.samples = torch.empty(self.n * samples, dtype=torch.uint8, device=dev)
        self.pixels = torch.empty(self.n * pixels, dtype=torch.uint8, device=dev)
        self.status = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.ws_bytes = max(int(L.acimg_png_unfilter_workspace(self.njobs)), int(L.acimg_png_pixels_workspace(self.n)))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)

    def unfilter(self):
        rc = self.L.acimg_png_unfilter(self.src.data_ptr(), self.src.numel(), self.jobs, self.njobs, self.n, self.samples.data_ptr(),
                                       self.samples.numel(), self.status.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self.st)
        assert rc == 0

    def to_pixels(self):
        rc = self.L.acimg_png_pixels(self.samples.data_ptr(), self.samples.numel(), self.files, self.n, None, 0,
                                     self.pixels.data_ptr(), self.pixels.numel(), self.status.data_ptr(), self.ws.data_ptr(),
                                     self.ws_bytes, self.st)
        assert rc == 0


def measure(dev, launch, a, want=None, pixels=False):
    launch.unfilter()
    launch.to_pixels()
    assert not launch.status.cpu().numpy().any(), "the bench files decode"
    if want is not None:
        assert np.array_equal(launch.pixels.cpu().numpy().reshape(want.shape), want), "the bench files give their pictures back"
    t = timed(dev, launch.unfilter, a.launches, a.repeats)
    out = dict(unfilter_us_per_launch=spread([x * 1e6 for x in t]), unfilter_files_per_s=spread([launch.n / x for x in t]))
    if pixels:
        t = timed(dev, launch.to_pixels, a.launches, a.repeats)
        out.update(pixels_us_per_launch=spread([x * 1e6 for x in t]), pixels_files_per_s=spread([launch.n / x for x in t]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--unique", type=int, default=8, help="pictures the Python writer filters; repeated to --files")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--tmp", type=str, default=None)
    a = ap.parse_args()
    import convert_ref
    import png_cases
    import png_writer
    from acimg import _lib, convert_collected

    dev = torch.device("cuda:0")
    L = _lib.load()
    n, unique = a.files, max(1, min(a.unique, a.files))
    rng = np.random.RandomState(0)
    pictures = [png_cases.photo(H, W, 40 + k) for k in range(unique)]
    want = np.stack([pictures[i % unique][..., ::-1] for i in range(n)])
    res = dict(height=H, width=W, files=n, unique=unique, repeats=a.repeats, launches=a.launches)

    # ---- the two kernels alone ------------------------------------------------------------------------------------------------
    variants = [("filter%d" % f, f, 0) for f in range(5)] + [("mixed", None, 0), ("adam7_mixed", None, 1)]
    mixed_files = None
    for name, filters, lace in variants:
        kinds = filters if filters is not None else tuple(int(v) for v in rng.randint(0, 5, size=H + 13))
        raws = [png_writer.scanlines(p.astype(np.uint16), 2, 8, kinds, lace) for p in pictures]
        launch = Launch(dev, L, [raws[i % unique] for i in range(n)], (H, W, 2, 8, lace))
        res[name] = measure(dev, launch, a, want, pixels=name in ("mixed", "adam7_mixed"))
        if name == "mixed":
            mixed_files = [png_writer.assemble(r, H, W, 2, 8) for r in raws]
    for rows in (1, 64, 65):
        pic = pictures[0][:rows].astype(np.uint16)
        raw = png_writer.scanlines(pic, 2, 8, tuple(int(v) for v in rng.randint(1, 5, size=rows)))
        res["one_file_rows%d" % rows] = measure(dev, Launch(dev, L, [raw], (rows, W, 2, 8, 0)), a, pictures[0][:rows][None, ..., ::-1])
    res["rows64_over_rows1"] = (res["one_file_rows64"]["unfilter_us_per_launch"]["median"]
                                / res["one_file_rows1"]["unfilter_us_per_launch"]["median"])
    res["rows65_over_rows1"] = (res["one_file_rows65"]["unfilter_us_per_launch"]["median"]
                                / res["one_file_rows1"]["unfilter_us_per_launch"]["median"])

    # ---- Pillow on the host, for scale ----------------------------------------------------------------------------------------
    files = [mixed_files[i % unique] for i in range(n)]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is None:
        res["pillow_16_threads_files_per_s"] = "Pillow was absent"
    else:
        def load(f):
            Image.open(io.BytesIO(f)).load()
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            list(pool.map(load, files))
            t0 = time.perf_counter()
            list(pool.map(load, files))
            res["pillow_16_threads_files_per_s"] = n / (time.perf_counter() - t0)

    # ---- end to end -------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="bench_convert_collected_", dir=a.tmp)
    try:
        raw, outd = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        os.makedirs(raw)
        rate, seconds = 44100, 10
        wav = convert_ref.wav_bytes((rng.randn(rate * seconds) * 3000).astype(np.int32), rate=rate)
        ids = range(1, len(convert_collected.CLASS_OF_ID) + 1)
        for i in ids:
            with open(os.path.join(raw, "%d.png" % i), "wb") as fh:
                fh.write(mixed_files[i % unique])
            with open(os.path.join(raw, "%d.wav" % i), "wb") as fh:
                fh.write(wav)
        with open(os.path.join(raw, "test_list.txt"), "w") as fh:
            fh.write("".join("%d.png\n" % i for i in ids))
        res["convert"] = {}
        for inflate in ("zlib", "device"):
            for deflate in ("zlib", "device"):
                rates, times = [], []
                for rep in range(a.repeats + 1):          # the first pass is the warm-up (page cache, code objects)
                    shutil.rmtree(outd, ignore_errors=True)
                    os.makedirs(outd)
                    t0 = time.perf_counter()
                    paths, conv = convert_collected.convert(raw, outd, device=str(dev), workers=a.workers, deflate=deflate,
                                                            inflate=inflate)
                    dt = time.perf_counter() - t0
                    if rep:
                        rates.append(len(paths) / dt)
                        times.append(dict(conv.times))
                res["convert"]["inflate_%s_deflate_%s" % (inflate, deflate)] = dict(
                    files=len(paths), workers=a.workers, clip_seconds=seconds, clip_rate=rate, files_per_s=spread(rates),
                    seconds={k: statistics.median(t[k] for t in times) for k in times[0]},
                    png_file_bytes=len(mixed_files[0]), record_file_bytes=os.path.getsize(paths[0]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
