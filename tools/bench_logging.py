"""Cost of the TensorBoard log of `Trainer.train()` on one GPU: three legs over the same synthetic batches (made once by
`SyntheticDataLoader`, kept on the device), alternating, --rounds times:

    none   trainer.logger = None (the loop as it was before the logger existed: this leg runs on an older tree too)
    log    a Logger: scalars + the eight device-rendered images on every displayed step
    hist   the same + one histogram per trainable variable (acimg_histogram_segments)

One epoch of --steps batches of --batch per leg and round; `train()`'s initialisation and its one-batch validation are
the same in every leg, so the legs' difference is the log.  Prints one JSON line per pass and a summary: per leg the
median and the spread of the epoch time, the two overheads in ms per displayed step, and the histogram launch sequence
alone (events around it, median of --hist_reps) against its HBM bound: the bytes of the trainable buffer over
--hbm_gbs (DESIGN §10's bandwidth).

    python tools/bench_logging.py --batch 32 --steps 100 --display_freq 50 --rounds 3 [--legs none,log,hist]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))

import torch  # noqa: E402


class Cached(object):
    """batches resident on the device, iterated like a loader"""

    def __init__(self, loader, device):
        self.batch_size = loader.batch_size
        self.batches = [tuple(t.to(device) for t in b) for b in loader.data]
        self.data = self.batches


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--display_freq", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", type=str, default="none,log,hist")
    ap.add_argument("--pipeline", type=int, default=1)
    ap.add_argument("--hist_reps", type=int, default=20)
    ap.add_argument("--hbm_gbs", type=float, default=5000.0)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args()

    from acimg.data import SyntheticDataLoader
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    device = torch.device(args.device)
    FLAGS.model, FLAGS.ae, FLAGS.exp_name, FLAGS.checkpoint_dir, FLAGS.pipeline = "UNet", 0, "bench_logging", None, args.pipeline
    FLAGS.restore_checkpoint = FLAGS.init_checkpoint = FLAGS.acoustic_init_checkpoint = FLAGS.visual_init_checkpoint = None
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), display_freq=args.display_freq,
                 num_epochs=1, session=Session(device))
    tr.log = lambda *a: None
    train = Cached(SyntheticDataLoader(args.steps * args.batch, args.batch), device)
    valid = Cached(SyntheticDataLoader(args.batch, args.batch, seed=99), device)
    legs = [x for x in args.legs.split(",") if x]
    displayed = -(-args.steps // args.display_freq)
    tmp = tempfile.mkdtemp(prefix="bench_logging_")
    times = dict((leg, []) for leg in legs)

    def one(leg, i):
        if leg != "none":
            from acimg.logger import Logger
            tr.logger = Logger(os.path.join(tmp, "%s%d" % (leg, i)))
            tr.log_histograms = leg == "hist"
        if tr.session.store.adam_m is not None:      # every pass starts where the first did: train() re-initialises the
            tr.session.store.adam_m.zero_()          # variables, not the optimiser's slots or the step counter
            tr.session.store.adam_v.zero_()
        tr.global_step = 0
        tr._noise_calls = 0                          # ... nor the eps counter: every pass draws the same noise
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        tr.train(train, valid)
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        if leg != "none":
            tr.logger.close()
            tr.logger = None
        return dt

    one(legs[0], -1)          # warm-up: plans, lanes, allocator
    for i in range(args.rounds):
        for leg in legs:
            dt = one(leg, i)
            times[leg].append(dt)
            print(json.dumps(dict(leg=leg, round=i, epoch_s=round(dt, 4), ms_per_step=round(1e3 * dt / args.steps, 3))))
    out = dict(batch=args.batch, steps=args.steps, display_freq=args.display_freq, displayed=displayed, pipeline=args.pipeline)
    for leg in legs:
        t = times[leg]
        out[leg] = dict(median_s=round(statistics.median(t), 4), min_s=round(min(t), 4), max_s=round(max(t), 4))
    for leg in legs:
        if leg != "none" and "none" in times:
            out[leg]["overhead_ms_per_displayed_step"] = round(
                1e3 * (statistics.median(times[leg]) - statistics.median(times["none"])) / displayed, 3)
    if "hist" in legs:
        from acimg import ops
        names, table, limits, total, _ = tr._histogram_table()
        V, L = len(names), limits.numel()
        counts = torch.empty((V, L), dtype=torch.int64, device=device)
        stats = torch.empty((V, 4), dtype=torch.float64, device=device)
        bad = torch.empty((V,), dtype=torch.int64, device=device)
        plan = ops.Plan(device, eager=True)
        ms = []
        for _ in range(args.hist_reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.histogram_segments(plan, tr.session.store.flat["train"], table, V, limits, L, total, counts, stats, bad)
            e1.record()
            torch.cuda.synchronize(device)
            ms.append(e0.elapsed_time(e1))
        ms = ms[3:]
        nbytes = 4 * tr.session.store.train_numel()
        bound_ms = 1e3 * nbytes / (args.hbm_gbs * 1e9)
        out["histogram_launch"] = dict(segments=len(names), read_floats=int(total), buffer_bytes=nbytes,
                                       median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                                       hbm_bound_ms=round(bound_ms, 4),
                                       fraction_of_bound=round(bound_ms / statistics.median(ms), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
