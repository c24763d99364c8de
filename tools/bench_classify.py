"""Time of the classification experiment on one GPU: the `TrainerClass` train step of its three sources (DualCamNet on
generated images, on real acoustic images, on the tiled MFCC map) at 2 and 5 clips of 12 frames, and one evaluation
pass of the baseline classifier in two forms - `ClipEvaluator` (forward plan + `acimg_clip_eval`, one read-back per
pass) against the per-batch form (`eval_step`: `g.out[:2].tolist()` after every batch).  Random variables and synthetic
batches resident on the device (the cost does not depend on the values); wall time around a synchronised loop, best and
median of --repeats.  Prints one JSON line per measurement.

    python tools/bench_classify.py --clips 2 5 --steps 30 --warmup 5 --batches 50
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


def build(source, clips, dev):
    from acimg.dualcamnet import DualCamHybridModel
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer_class import TrainerClass
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    FLAGS.model, FLAGS.ae = "DualCamNet", 0
    mi = ma = None
    if source == "generated":
        mi = ResNet50Model(input_shape=[224, 298, 3], num_classes=None)
        ma = UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1)
    tr = TrainerClass(DualCamHybridModel(input_shape=[36, 48, 12], num_classes=10), mi, ma, learning_rate=1e-3,
                      num_classes=10, session=Session(dev), source=source)
    tr.log = lambda *a: None
    tr._build_functions(batch_size=clips * 12)
    tr._initialize()
    return tr


def batch_for(source, clips, dev, gen):
    n = clips * 12
    labels = torch.randint(0, 10, (clips,), generator=gen).to(dev)
    ac = torch.rand(n, 36, 48, 12, generator=gen).to(dev) if source == "acoustic" else None
    mfcc = torch.rand(n, 12, generator=gen).to(dev)
    video = torch.rand(n, 224, 298, 3, generator=gen).to(dev) if source == "generated" else None
    return (ac, mfcc, video, labels)


def timed(fn, repeats, dev):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append(time.perf_counter() - t0)
    return min(out), statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=50, help="batches of one evaluation pass")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    for source in ("generated", "acoustic", "mfccmap"):
        for clips in a.clips:
            tr = build(source, clips, dev)
            batch = batch_for(source, clips, dev, gen)
            tr.train_step(batch)

            def steps(n=a.steps):
                for _ in range(n):
                    tr.train_step(None)
            steps(a.warmup)
            best, med = timed(steps, a.repeats, dev)
            print(json.dumps(dict(what="train_step", source=source, clips=clips, frames=clips * 12, steps=a.steps,
                                  steps_per_s=a.steps / best, frames_per_s=a.steps * clips * 12 / best,
                                  steps_per_s_median=a.steps / med, ms_per_step=1e3 * best / a.steps)), flush=True)
            if source != "acoustic":
                continue
            g = tr.primary
            tr._feed(g, batch, None)

            def pass_device():
                tr._begin_pass()
                for _ in range(a.batches):
                    g.plan_pass.run()
                return tr._end_pass()

            def pass_per_batch():
                loss = acc = 0.0
                for _ in range(a.batches):
                    r = tr.eval_step(None)
                    loss += r["loss"] * g.clips
                    acc += r["accuracy"] * g.clips
                return loss, acc
            for name, fn in (("ClipEvaluator", pass_device), ("per_batch_tolist", pass_per_batch)):
                fn()
                best, med = timed(fn, a.repeats, dev)
                print(json.dumps(dict(what="evaluation_pass", form=name, source=source, clips=clips, batches=a.batches,
                                      ms_per_pass=1e3 * best, ms_per_pass_median=1e3 * med,
                                      ms_per_batch=1e3 * best / a.batches)), flush=True)


if __name__ == "__main__":
    main()
