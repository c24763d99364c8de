"""The box-record converter on one GPU, at the data set's geometry (256 x 256 JPEG files, 4:2:0 -> 224 x 298):

* the three decode stages alone (`acimg_jpeg_decode_entropy`, `_idct`, `_colour`) at --files files per launch: --launches
  back-to-back launches between two device events, --repeats times after a warm-up; files/s each.  The files come from
  this project's own encoder (`acimg.jpeg.JpegEncoder`, quality 90), once WITHOUT restart markers - what a camera or an
  imaging library writes, one lane per file in the entropy stage - and once with one restart interval per MCU row (16 per
  file, 16 lanes per file): the ratio of the two entropy rates is what the one-lane-per-interval shape costs on files
  without restart markers.
* the resampler alone (`acimg_resample_sinc`) on one 10 s clip at 44100 Hz: clips/s and output samples/s.
* the converter end to end (`acimg.convert_boxes.convert`) on a tree of --files files written to --tmp: files/s of wall
  time, and where the time goes: `read`, `parse` and `deflate` are summed over the --workers threads, `device` (upload +
  decode + resize + resample + download) is wall time of the calling thread.  `--deflate device` compresses the records
  on the GPU (acimg.deflate) instead of gzip level 9 on the workers; tools/bench_deflate.py runs both alternately.
* where Pillow is importable, its decode rate of the same files on one host thread, for scale.
* `--progressive`: instead of the above, the same pictures' coefficients re-written as progressive files (the writer of
  tests/jpeg_progressive_writer.py with Pillow's ten-scan script, with and without restart intervals):
  `acimg_jpeg_decode_progressive` beside `acimg_jpeg_decode_entropy` on the same coefficients, the items and busy lanes of
  each level, and the converter end to end on the progressive files.
Prints one JSON line.

    python tools/bench_convert_boxes.py --files 256 --workers 4 --repeats 5
    python tools/bench_convert_boxes.py --progressive --files 256 --workers 4 --repeats 5
"""
import argparse
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

SIDE = 256


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def photo_like(rng, n):
    """smooth structure plus sensor noise"""
    coarse = rng.randint(0, 256, size=(n, SIDE // 8, SIDE // 8, 3)).astype(np.float32)
    smooth = np.kron(coarse, np.ones((1, 8, 8, 1), np.float32))
    return np.clip(smooth + rng.normal(0, 3, size=smooth.shape), 0, 255).astype(np.uint8)


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


def write_tree(raw, jpegs, clip, rate):
    """ROOT/test_list.txt, Dataset/Data/0/<id>.{jpg,wav}, Dataset/Annotations/<id>.xml: one file per JPEG, all with `clip`"""
    import convert_boxes_support as support
    import convert_ref
    data_dir, ann_dir = os.path.join(raw, "Dataset", "Data", "0"), os.path.join(raw, "Dataset", "Annotations")
    os.makedirs(data_dir)
    os.makedirs(ann_dir)
    names = []
    wav = convert_ref.wav_bytes(clip, rate=rate)
    for i, f in enumerate(jpegs):
        ident = "%06d" % i
        names.append(ident + ".jpg")
        with open(os.path.join(data_dir, ident + ".jpg"), "wb") as fh:
            fh.write(f)
        with open(os.path.join(data_dir, ident + ".wav"), "wb") as fh:
            fh.write(wav)
        with open(os.path.join(ann_dir, ident + ".xml"), "wb") as fh:
            fh.write(support.annotation_xml(ident, [("object", 40, 50, 200, 220)]))
    with open(os.path.join(raw, "test_list.txt"), "w") as fh:
        fh.write("".join(nm + "\n" for nm in names))


def progressive_mode(a, dev, L, encoded, clip, rate):
    """--progressive: the coefficients of the same pictures re-written as progressive files (tests/jpeg_progressive_writer.py,
    Pillow's ten-scan script) without restart markers and with an interval of 16 (one MCU row in the DC scans, 16 blocks in
    the AC scans); the progressive entropy stage beside the baseline one on the same coefficients, the lanes each level
    keeps busy, and the converter end to end on the progressive files.  The writer is Python, so --unique pictures are
    re-written and repeated to --files a launch."""
    import jpeg_progressive_writer as pw
    from acimg import convert_boxes, jpeg, ops
    n, st = a.files, ops.current_stream_handle(dev)
    dec = jpeg.JpegDecoder(dev)
    unique = max(1, min(a.unique, n))
    base_files = {k: [v[i % unique] for i in range(n)] for k, v in encoded.items()}
    infos = [jpeg.parse_jpeg(f) for f in base_files["no_restart"][:unique]]
    g = infos[0]
    geo = (g.height, g.width, g.comps, g.hs, g.vs)
    coef = dec.stages(base_files["no_restart"][:unique], infos)[0].cpu().numpy()
    t0 = time.perf_counter()
    written = {key: [pw.write(coef[i], infos[i].quant, geo, pw.PILLOW_SCRIPT_3, restart) for i in range(unique)]
               for key, restart in (("no_restart", 0), ("restart_16", 16))}
    res = dict(side=SIDE, files=n, unique=unique, repeats=a.repeats, launches=a.launches, writer_seconds=time.perf_counter() - t0)
    res["file_bytes"] = {k: int(statistics.median(len(f) for f in v)) for k, v in written.items()}
    out = torch.empty(n, g.mcus, g.blocks, 64, dtype=torch.int16, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    want = torch.from_numpy(coef).to(dev)
    for key, files in base_files.items():                  # the baseline stage on the same coefficients
        bi = [jpeg.parse_jpeg(f) for f in files]
        data, desc, intervals, huff, _ = dec.upload(files, bi)
        call = lambda: L.acimg_jpeg_decode_entropy(data.data_ptr(), data.numel(), desc.data_ptr(), intervals.data_ptr(),  # noqa: E731
                                                   intervals.shape[0], huff.data_ptr(), n, *geo, out.data_ptr(), out.numel() * 2,
                                                   status.data_ptr(), st)
        t = timed(dev, call, a.launches, a.repeats)
        assert not status.cpu().numpy().any() and torch.equal(out[:unique], want)
        res["baseline_entropy_" + key] = dict(intervals_per_file=len(bi[0].intervals), ms_per_launch=spread([x * 1e3 for x in t]),
                                              files_per_s=spread([n / x for x in t]))
    for key, some in written.items():
        files = [some[i % unique] for i in range(n)]
        pi = [jpeg.parse_jpeg(f) for f in files]
        data, img, scans, intervals, huff, _ = dec.upload(files, pi)
        call = lambda: L.acimg_jpeg_decode_progressive(data.data_ptr(), data.numel(), img.data_ptr(), scans.data_ptr(),  # noqa: E731
                                                       scans.shape[0], intervals.data_ptr(), intervals.shape[0], huff.data_ptr(),
                                                       huff.shape[0], n, *geo, out.data_ptr(), out.numel() * 2,
                                                       status.data_ptr(), st)
        t = timed(dev, call, a.launches, a.repeats)
        assert not status.cpu().numpy().any() and torch.equal(out[:unique], want), "the progressive files give the coefficients back"
        # where the time goes: Pillow's script has its levels in file order, so a launch on the first 5 and the first 9 scans
        # of every file (a record count is all that changes) is a launch of level 0 and of levels 0 and 1
        order = [s.level for s in pi[0].scans]
        assert order == sorted(order)
        upto = {}
        for level in sorted(set(order))[:-1]:
            img_cut = img.clone()
            img_cut[:, 3] = sum(1 for v in order if v <= level)
            cut = lambda: L.acimg_jpeg_decode_progressive(data.data_ptr(), data.numel(), img_cut.data_ptr(), scans.data_ptr(),  # noqa: E731
                                                          scans.shape[0], intervals.data_ptr(), intervals.shape[0],
                                                          huff.data_ptr(), huff.shape[0], n, *geo, out.data_ptr(),
                                                          out.numel() * 2, status.data_ptr(), st)
            upto[level] = statistics.median(timed(dev, cut, a.launches, a.repeats)) * 1e3
            assert not status.cpu().numpy().any()
        upto[max(order)] = statistics.median(t) * 1e3
        levels = {}
        for s in pi[0].scans:
            levels.setdefault(s.level, [0, 0, 0])
            levels[s.level][0] += 1
            levels[s.level][1] += s.count
            levels[s.level][2] += s.end - s.begin
        res["progressive_entropy_" + key] = dict(
            ms_per_launch=spread([x * 1e3 for x in t]), files_per_s=spread([n / x for x in t]),
            levels=[dict(level=k, scans=v[0], items=v[1], lanes_busy=min(v[1], 64), bytes=v[2], ms_up_to_here=upto[k])
                    for k, v in sorted(levels.items())])
    tmp = tempfile.mkdtemp(prefix="bench_convert_boxes_", dir=a.tmp)
    try:
        for key, some in written.items():
            raw, outd = os.path.join(tmp, key, "raw"), os.path.join(tmp, key, "out")
            write_tree(raw, [some[i % unique] for i in range(n)], clip, rate)
            rates, shares = [], []
            for rep in range(a.repeats + 1):
                shutil.rmtree(outd, ignore_errors=True)
                os.makedirs(outd)
                t0 = time.perf_counter()
                paths, conv = convert_boxes.convert(raw, outd, device=str(dev), workers=a.workers, deflate=a.deflate)
                dt = time.perf_counter() - t0
                if rep:
                    rates.append(len(paths) / dt)
                    tot = sum(conv.times.values())
                    shares.append({k: v / tot for k, v in conv.times.items()})
            res["convert_progressive_" + key] = dict(files=n, workers=a.workers, deflate=a.deflate, files_per_s=spread(rates),
                                                     share={k: statistics.median(s[k] for s in shares) for k in shares[0]})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--progressive", action="store_true", help="measure the progressive entropy stage and converter instead")
    ap.add_argument("--unique", type=int, default=16, help="--progressive: pictures the Python writer re-writes")
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--tmp", type=str, default=None)
    ap.add_argument("--deflate", default="zlib", choices=("zlib", "device"))
    a = ap.parse_args()
    from acimg import _lib, convert_boxes, jpeg, ops

    dev = torch.device("cuda:0")
    L = _lib.load()
    rng = np.random.RandomState(0)
    n = a.files
    res = dict(side=SIDE, files=n, repeats=a.repeats, launches=a.launches)
    frames = torch.from_numpy(photo_like(rng, n))
    mcus = (SIDE // 16) ** 2
    encoded = {"no_restart": jpeg.JpegEncoder(dev, 90, restart_mcus=mcus).encode(frames),
               "restart_per_mcu_row": jpeg.JpegEncoder(dev, 90).encode(frames)}
    res["file_bytes"] = {k: int(statistics.median(len(f) for f in v)) for k, v in encoded.items()}
    if a.progressive:
        return progressive_mode(a, dev, L, encoded, (rng.randn(44100 * 10) * 3000).astype(np.int32), 44100)

    # ---- the decode stages alone ----------------------------------------------------------------------------------------------
    dec = jpeg.JpegDecoder(dev)
    st = ops.current_stream_handle(dev)
    for key, files in encoded.items():
        infos = [jpeg.parse_jpeg(f) for f in files]
        g = infos[0]
        geo = (g.height, g.width, g.comps, g.hs, g.vs)
        data, desc, intervals, huff, quant = dec.upload(files, infos)
        coef, planes, bgr, status = dec.stages(files, infos)
        assert not status.cpu().numpy().any(), "the bench files decode"
        calls = dict(
            entropy=lambda: L.acimg_jpeg_decode_entropy(data.data_ptr(), data.numel(), desc.data_ptr(), intervals.data_ptr(),
                                                        intervals.shape[0], huff.data_ptr(), n, *geo, coef.data_ptr(),
                                                        coef.numel() * 2, status.data_ptr(), st),
            idct=lambda: L.acimg_jpeg_decode_idct(coef.data_ptr(), quant.data_ptr(), n, *geo, planes.data_ptr(), planes.numel(), st),
            colour=lambda: L.acimg_jpeg_decode_colour(planes.data_ptr(), n, *geo, bgr.data_ptr(), bgr.numel(), st))
        stages = {}
        for name, call in calls.items():
            if key != "no_restart" and name != "entropy":
                continue                                   # the later stages do not see the restart markers
            t = timed(dev, call, a.launches, a.repeats)
            stages[name] = dict(ms_per_launch=spread([x * 1e3 for x in t]), files_per_s=spread([n / x for x in t]))
        res["decode_" + key] = dict(intervals_per_file=len(g.intervals), **stages)
    res["entropy_cost_of_one_lane_per_file"] = (res["decode_no_restart"]["entropy"]["ms_per_launch"]["median"]
                                                / res["decode_restart_per_mcu_row"]["entropy"]["ms_per_launch"]["median"])

    # ---- the resampler alone ------------------------------------------------------------------------------------------------
    rate, seconds = 44100, 10
    clip = (rng.randn(rate * seconds) * 3000).astype(np.int32)
    rs = convert_boxes.Resampler(dev)
    x = torch.from_numpy(clip).to(dev)
    y, _ = rs.resample_device(x, rate)
    t = timed(dev, lambda: rs.resample_device(x, rate), a.launches, a.repeats)
    res["resample_10s_44100"] = dict(ms_per_clip=spread([v * 1e3 for v in t]),
                                     output_samples_per_s=spread([y.numel() / v for v in t]))

    # ---- Pillow on the host, for scale ----------------------------------------------------------------------------------------
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        t0 = time.perf_counter()
        for f in encoded["no_restart"]:
            np.asarray(Image.open(io.BytesIO(f)))
        res["pillow_one_thread_files_per_s"] = n / (time.perf_counter() - t0)

    # ---- end to end -------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="bench_convert_boxes_", dir=a.tmp)
    try:
        raw, outd = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        write_tree(raw, encoded["no_restart"], clip, rate)
        rates, shares = [], []
        for rep in range(a.repeats + 1):          # the first pass is the warm-up (page cache, code objects)
            shutil.rmtree(outd, ignore_errors=True)
            os.makedirs(outd)
            t0 = time.perf_counter()
            paths, conv = convert_boxes.convert(raw, outd, device=str(dev), workers=a.workers, deflate=a.deflate)
            dt = time.perf_counter() - t0
            if rep:
                rates.append(len(paths) / dt)
                tot = sum(conv.times.values())
                shares.append({k: v / tot for k, v in conv.times.items()})
        res["convert"] = dict(files=n, workers=a.workers, deflate=a.deflate, clip_seconds=seconds, clip_rate=rate, files_per_s=spread(rates),
                              share={k: statistics.median(s[k] for s in shares) for k in shares[0]},
                              record_file_bytes=os.path.getsize(paths[0]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
