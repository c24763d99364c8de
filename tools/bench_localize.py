"""Time per batch of the Flickr-SoundNet localisation evaluation on one GPU: `Trainer.generate` (the inference-mode
forward of ResNet50Model + UNetAc) and the box metric after it (`BoxIoU.iou`: find_logen + acimg_box_iou), each timed
with CUDA events over --steps batches after --warmup.  Random variables and synthetic batches (the cost does not depend
on the values).  Prints one JSON line per batch size.

    python tools/bench_localize.py --batch 32 64 --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from acimg.evaluate import BoxIoU
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    dev = torch.device("cuda:0")
    FLAGS.model, FLAGS.ae = "UNet", 0
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(dev))
    tr._build_functions(batch_size=a.batch[0])
    tr.modelimages.initialize()
    tr.modelac.initialize()
    metric = BoxIoU(dev)
    g = torch.Generator().manual_seed(0)
    for n in a.batch:
        batch = (torch.zeros(n, 36, 48, 12), torch.rand(n, 12, generator=g), torch.rand(n, 224, 298, 3, generator=g))
        boxes = torch.randint(0, 298, (n, 4, 3), generator=g, dtype=torch.int32).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_gen = t_met = 0.0
        for i in range(a.warmup + a.steps):
            ev[0].record()
            out = tr.generate(batch)
            ev[1].record()
            metric.iou(out, boxes)
            ev[2].record()
            torch.cuda.synchronize(dev)
            if i >= a.warmup:
                t_gen += ev[0].elapsed_time(ev[1])
                t_met += ev[1].elapsed_time(ev[2])
        print(json.dumps(dict(batch=n, generate_ms=t_gen / a.steps, metric_ms=t_met / a.steps,
                              metric_fraction=t_met / t_gen, steps=a.steps)))


if __name__ == "__main__":
    main()
