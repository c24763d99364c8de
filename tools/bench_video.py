"""What `python -m acimg.show video` does with a rendered batch, on one GPU: the PNG path as it stands (the batch copied
to the host, every frame deflated by `acimg.png.encode_png`) beside the JPEG path of `--avi 1` (`JpegEncoder.encode`: two
kernels, the byte counts and the packed scans read back), at 224 x 298, --frames frames in batches of --batch.  The frames
are overlays rendered by `OverlayRenderer` (a smooth energy map over noise frames): the cost of both paths depends on the
content.  Each path runs --repeats times over all frames after --warmup batches; the rates are frames per second of
host wall time (the paths end in a device -> host copy, which synchronises); the two kernels' device time per batch is
taken from events around each C-ABI call.  Nothing is written to disk.  Prints one JSON line.

    python tools/bench_video.py --frames 240 --batch 12 --repeats 5 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))

import torch  # noqa: E402


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--restart_mcus", type=int, default=None)
    ap.add_argument("--png_level", type=int, default=6)
    a = ap.parse_args()
    import numpy as np

    from acimg import _lib, ops
    from acimg.evaluate import OverlayRenderer
    from acimg.jpeg import JpegEncoder
    from acimg.png import encode_png

    dev = torch.device("cuda:0")
    L = _lib.load()
    rend = OverlayRenderer(dev)
    enc = JpegEncoder(dev, a.quality, a.restart_mcus)
    g = torch.Generator().manual_seed(0)
    n, H, W = a.batch, 224, 298
    hann = torch.outer(torch.hann_window(36, periodic=False), torch.hann_window(48, periodic=False))
    batches = []
    for b in range(a.frames // n):
        frames = torch.rand(n, H, W, 3, generator=g).to(dev)
        energy = (hann.reshape(1, -1) * (0.5 + torch.rand(n, 1, generator=g)) + 0.01 * torch.rand(n, 36 * 48, generator=g)).to(dev)
        batches.append(rend.render(frames, energy))
    torch.cuda.synchronize(dev)
    total = len(batches) * n

    def png_pass(bs):
        nbytes = 0
        for img in bs:
            host = img.cpu().numpy()
            for h in range(host.shape[0]):
                nbytes += len(encode_png(host[h], a.png_level))
        return nbytes

    def jpeg_pass(bs):
        return sum(len(f) for img in bs for f in enc.encode(img))

    res = dict(frames=total, batch=n, height=H, width=W, quality=a.quality, restart_mcus=enc.restart_mcus(W),
               png_level=a.png_level, repeats=a.repeats)
    for name, fn in (("png", png_pass), ("jpeg", jpeg_pass)):
        fn(batches[:a.warmup])
        rates = []
        for _ in range(a.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            nbytes = fn(batches)
            rates.append(total / (time.perf_counter() - t0))
        res[name + "_frames_per_s"] = spread(rates)
        res[name + "_file_bytes_per_frame"] = nbytes // total
    res["png_readback_bytes_per_frame"] = H * W * 3

    # the two kernels alone: events around each call, per batch
    r = enc.restart_mcus(W)
    stride = -(-int(L.acimg_jpeg_scan_capacity(H, W, r)) // 16) * 16
    coef = torch.empty(int(L.acimg_jpeg_coef_bytes(n, H, W)) // 2, dtype=torch.int16, device=dev)
    wsb = int(L.acimg_jpeg_scan_workspace(n, H, W, r))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(n, stride, dtype=torch.uint8, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    st = ops.current_stream_handle(dev)
    t_blocks, t_scan, scan_bytes = [], [], []
    for rep in range(a.repeats + 1):
        for img in batches:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            _lib.check(L.acimg_jpeg_blocks(img.data_ptr(), n, H, W, enc._qt_dev.data_ptr(), coef.data_ptr(), st), "jpeg_blocks")
            ev[1].record()
            _lib.check(L.acimg_jpeg_scan(coef.data_ptr(), n, H, W, r, out.data_ptr(), stride, cnt.data_ptr(), ws.data_ptr(),
                                         wsb, st), "jpeg_scan")
            ev[2].record()
            torch.cuda.synchronize(dev)
            if rep:                                          # the first sweep is the warm-up
                t_blocks.append(ev[0].elapsed_time(ev[1]) * 1e3)
                t_scan.append(ev[1].elapsed_time(ev[2]) * 1e3)
                scan_bytes.append(int(cnt.sum()))
    res["blocks_us_per_batch"] = spread(t_blocks)
    res["scan_us_per_batch"] = spread(t_scan)
    res["jpeg_readback_bytes_per_frame"] = int(np.mean(scan_bytes)) // n + 4
    res["readback_ratio"] = res["png_readback_bytes_per_frame"] / res["jpeg_readback_bytes_per_frame"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
