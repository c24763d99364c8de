"""Sound-source localisation evaluation of a trained generator: `python -m acimg.localize`.

Stands where the reference's two evaluation scripts stand, with their flags:
* `--datatype flickr`: showimages_bb.py (Flickr-SoundNet, box-annotated records, `BoxRecordLoader`): the generated
  image's energy-map mask, resized to the frame, against the annotators' consensus boxes (`BoxIoU`, :286-320);
* `--datatype outdoor` (any other value): iouenergythreshold.py (records of `TFRecordDataLoader`): the generated image's
  mask against the real acoustic image's (`EnergyIoU`, :213-229).
Both build ResNet50Model + UNetAc(num_skip), restore the Saver-V2 checkpoint `--init_checkpoint` (every model variable,
as `tf.train.Saver(var_list).restore` does, :130-134), and stream the data set through `Trainer.generate` (inference
mode: BN moving statistics, keep_prob 1).  Output, next to the checkpoint in the directory the scripts name:
* `intersection_<tau>_accuracy.txt` = 'iou {:6f}' of the fraction of samples with IoU > tau (showimages_bb.py:327-328,
  iouenergythreshold.py:229-230), for every tau of the 11-point curve (and --threshold if it is not one of them) - the
  files areaundercurve.py reads;
* `localization.json`: the per-sample IoUs (NaN -> null), the 11-point curve, its area (areaundercurve.py:26-40), the
  mean IoU over the finite samples and the NaN count.
The pictures of the same scripts - the energy map over the frame, with the boxes - are `python -m acimg.show`."""
import argparse
import json
import math
import os
import sys

import numpy as np

from .evaluate import THRESHOLDS, accuracy_curve, area_under_curve, mean_iou

RESULT_FILE = "localization.json"


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m acimg.localize", description=__doc__.split("\n")[0])
    ap.add_argument("--model", type=str, default="UNet", help="model type (UNet)")
    ap.add_argument("--train_file", type=str, required=True, help="text file listing the TFRecord files")
    ap.add_argument("--init_checkpoint", type=str, required=True, help="Saver-V2 checkpoint prefix (.../epoch_N.ckpt)")
    ap.add_argument("--batch_size", type=int, default=2)
    ap.add_argument("--num_skip_conn", type=int, default=1, choices=(0, 1, 2))
    ap.add_argument("--ae", type=int, default=0, help="1: plain auto-encoder generator (no sampling)")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--datatype", type=str, default="flickr", help="flickr: box metric; outdoor: energy metric")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def is_box_metric(args):
    return args.datatype == "flickr"


def output_dir(args):
    """<checkpoint dir>/<model>_<data set>_<tag>_<checkpoint number> (showimages_bb.py:41-47: tag AcousticFramesJet2;
    iouenergythreshold.py:40-46: tag Acoustictry)"""
    dataset = args.train_file.split("/")[-1].split(".")[0]
    base = args.init_checkpoint.split("/")[-1]
    parts = base.split("_")
    name = (parts[1] if len(parts) > 1 else base).split(".ckpt")[0]
    tag = "AcousticFramesJet2" if is_box_metric(args) else "Acoustictry"
    name = "{}_{}_{}_{}".format(args.model, dataset, tag, name)
    return "/".join(args.init_checkpoint.split("/")[:-1] + [name])


def accuracy_file(data_dir, tau):
    return os.path.join(data_dir, "intersection_{}_accuracy.txt".format(tau * 1.0))


def write_outputs(data_dir, ious, threshold=0.5, extra=None):
    """the reference's accuracy files + the JSON summary; returns the summary dict"""
    os.makedirs(data_dir, exist_ok=True)
    ious = np.asarray(ious, dtype=np.float64)
    taus = list(THRESHOLDS) + ([float(threshold)] if float(threshold) not in THRESHOLDS else [])
    acc = accuracy_curve(ious, taus)
    for tau, a in zip(taus, acc):
        with open(accuracy_file(data_dir, tau), "w") as f:
            f.write("iou {:6f}".format(a))
    curve = [float(a) for a in acc[:len(THRESHOLDS)]]
    miou, nans = mean_iou(ious)
    res = dict(num_samples=int(ious.size), thresholds=list(THRESHOLDS), accuracy=curve,
               auc=area_under_curve(curve), mean_iou=None if math.isnan(miou) else miou, nan_count=nans,
               threshold=float(threshold), accuracy_at_threshold=float(acc[taus.index(float(threshold))]),
               iou=[None if math.isnan(v) else float(v) for v in ious])
    res.update(extra or {})
    with open(os.path.join(data_dir, RESULT_FILE), "w") as f:
        json.dump(res, f, indent=1)
    return res


def build_trainer(args, device):
    """ResNet50Model + UNetAc(num_skip) in a Trainer sized for --batch_size, variables restored from the checkpoint"""
    from .flags import FLAGS
    from .session import Session
    from .trainer import Trainer
    from .unet_acresnet import UNetAc
    from .vision import ResNet50Model, load_state_file
    if args.model != "UNet":
        raise ValueError("Unknown model type %r" % args.model)
    FLAGS.model, FLAGS.ae, FLAGS.num_skip_conn = args.model, int(args.ae), int(args.num_skip_conn)
    sess = Session(device)
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=bool(args.ae), num_skip=args.num_skip_conn),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=sess)
    tr._build_functions(batch_size=args.batch_size)
    tr.session.store.load_state(load_state_file(args.init_checkpoint), strict=True)
    return tr


def run(args, trainer=None, keep_generated=False, log=print):
    """evaluate; returns the summary dict (+ 'generated': [n,36,48,12] float32 host array when keep_generated)"""
    import torch

    from .data import BoxRecordLoader, TFRecordDataLoader
    from .evaluate import BoxIoU, EnergyIoU
    device = torch.device(args.device)
    tr = trainer if trainer is not None else build_trainer(args, device)
    box = is_box_metric(args)
    if box:
        data = BoxRecordLoader(args.train_file, args.batch_size)
        metric = BoxIoU(device)
    else:
        data = TFRecordDataLoader(args.train_file, args.batch_size, device=device)
        metric = EnergyIoU(device)
    ious, kept = [], []
    for batch in data.data:
        out = tr.generate(batch)
        if box:
            boxes = torch.stack(list(batch[3:7]), 1)               # [n,4,3]: xmin, xmax, ymin, ymax
            ious.append(metric.iou64(out, boxes))
        else:
            real = batch[0].to(device, non_blocking=True).reshape(out.shape)
            ious.append(metric.iou(real, out).double().cpu().numpy())
        if keep_generated:
            kept.append(out.cpu().numpy())
        log("{} samples".format(sum(len(v) for v in ious)))
    ious = np.concatenate(ious) if ious else np.zeros(0)
    if ious.size == 0:
        raise ValueError("no samples in %s" % args.train_file)
    res = write_outputs(output_dir(args), ious, args.threshold,
                        extra=dict(datatype=args.datatype, metric="box" if box else "energy",
                                   checkpoint=args.init_checkpoint))
    log("iou {:6f} at threshold {}; area {:6f}; mean iou {} ({} NaN)".format(
        res["accuracy_at_threshold"], args.threshold, res["auc"], res["mean_iou"], res["nan_count"]))
    if keep_generated:
        res["generated"] = np.concatenate(kept)
    return res


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
