"""Time per batch of the localisation overlay on one GPU: `acimg_overlay_render` (its two launches, CUDA events over
--steps calls after --warmup) beside `Trainer.generate` of the same batch (the inference-mode forward of ResNet50Model +
UNetAc), beside the NumPy restatement of the same rule per frame on the host (tests/render_ref.py), and beside what the
command line does after the render: the copy to the host and the PNG compression per frame.  Random variables and
synthetic batches (the cost does not depend on the values).  Prints one JSON line per batch size.

    python tools/bench_show.py --batch 32 64 --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--png_level", type=int, default=6)
    ap.add_argument("--png_deflate", default="zlib", choices=("zlib", "device"), help="device: acimg.deflate codes the PNG rows")
    ap.add_argument("--no_generator", action="store_true", help="time the render alone (a kernel-trace run)")
    a = ap.parse_args()
    import numpy as np

    import render_ref
    from acimg import colormaps, ops
    from acimg.evaluate import OverlayRenderer
    from acimg.png import encode_png, encode_png_many

    dev = torch.device("cuda:0")
    tr = None
    if not a.no_generator:
        from acimg.flags import FLAGS
        from acimg.session import Session
        from acimg.trainer import Trainer
        from acimg.unet_acresnet import UNetAc
        from acimg.vision import ResNet50Model
        FLAGS.model, FLAGS.ae = "UNet", 0
        tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                     ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(dev))
        tr._build_functions(batch_size=a.batch[0])
        tr.modelimages.initialize()
        tr.modelac.initialize()
    rend = OverlayRenderer(dev)
    deflater = None
    if a.png_deflate == "device":
        from acimg.deflate import DeviceDeflater
        deflater = DeviceDeflater(dev)
    g = torch.Generator().manual_seed(0)
    for n in a.batch:
        batch = (torch.zeros(n, 36, 48, 12), torch.rand(n, 12, generator=g), torch.rand(n, 224, 298, 3, generator=g))
        frames = batch[2].to(dev)
        logen = (torch.rand(n, 36 * 48, generator=g) * 1e-3 + 0.04).to(dev)
        out = torch.empty(n, 224, 298, 3, dtype=torch.uint8, device=dev)
        plan = ops.Plan(dev)                                    # the recorded form: one ctypes call, two launches
        ops.overlay_render(plan, frames, 3, logen, None, rend.lut_base, rend.lut_over, 7, 10, out, 894, 224 * 894, n)
        plan.finalize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_gen = t_ren = 0.0
        for i in range(a.warmup + a.steps):
            ev[0].record()
            if tr is not None:
                tr.generate(batch)
            ev[1].record()
            plan.run()
            ev[2].record()
            torch.cuda.synchronize(dev)
            if i >= a.warmup:
                t_gen += ev[0].elapsed_time(ev[1])
                t_ren += ev[1].elapsed_time(ev[2])
        res = dict(batch=n, render_ms=t_ren / a.steps, steps=a.steps)
        if tr is not None:
            res.update(generate_ms=t_gen / a.steps, render_fraction=t_ren / t_gen)
        # the host side, per frame: device -> host copy, the NumPy restatement, the PNG compression
        t0 = time.perf_counter()
        host = out.cpu().numpy()
        t1 = time.perf_counter()
        k = min(n, 8)
        fr, lg = batch[2][:k].numpy(), logen[:k].cpu().numpy().reshape(k, 36, 48)
        gray, jet = colormaps.byte_table("gray"), colormaps.byte_table("jet")
        render_ref.render(fr[0], lg[0], gray, jet)              # first call: NumPy's own warm-up, not timed
        t2 = time.perf_counter()
        same = all(np.array_equal(render_ref.render(fr[j], lg[j], gray, jet), host[j]) for j in range(k))
        t3 = time.perf_counter()
        if deflater is not None:
            encode_png(host[0], deflater=deflater)              # first call: code object and allocator warm-up, not timed
            t3 = time.perf_counter()
        nbytes = sum(len(encode_png(host[j], a.png_level, deflater)) for j in range(k))
        t4 = time.perf_counter()
        if deflater is not None:      # what show.py's device branch calls: the batch from the device tensor, one call
            encode_png_many(out[:k], deflater)
            t5 = time.perf_counter()
            many = encode_png_many(out[:k], deflater)
            res.update(png_many_ms_per_frame=(time.perf_counter() - t5) * 1e3 / k,
                       png_many_equals_per_frame=many == [encode_png(host[j], deflater=deflater) for j in range(k)])
        res.update(copy_ms_per_frame=(t1 - t0) * 1e3 / n, numpy_ms_per_frame=(t3 - t2) * 1e3 / k,
                   png_ms_per_frame=(t4 - t3) * 1e3 / k, png_bytes_per_frame=nbytes // k, png_level=a.png_level, png_deflate=a.png_deflate,
                   matches_numpy=bool(same))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
