"""Latent-feature extraction of a trained generator: `python -m acimg.features`.

Stands where the reference's extract_features_unetraces.py stands, with its flags: ResNet50Model + UNetAc(num_skip)
restored from the Saver-V2 checkpoint `--init_checkpoint` (every model variable, :130-134), the records of
`--train_file` streamed once in order through the inference-mode forward (`Trainer.features`: BN moving statistics,
keep_prob 1), and for every frame the latent the decoder consumes, guessed_z = mean + std * eps (:124-125), with eps
drawn from a generator seeded by `--seed`.  Output, next to the checkpoint (:39-45, :182-184):

    <checkpoint dir>/<dataset>_<encoder_type>_<n>/<dataset>_data.npy       float64 [N,150]
    <checkpoint dir>/<dataset>_<encoder_type>_<n>/<dataset>_labels.npy     int one-hot [N,10]
    <checkpoint dir>/<dataset>_<encoder_type>_<n>/<dataset>_scenario.npy   int one-hot [N,61]

with <dataset> the list file's base name up to its first dot and <n> the checkpoint number: exactly what
`python -m acimg.retrieval knn | retrieve` read.  `--ae 1` saves the auto-encoder's code itself; the reference script
reads `model.std`, which that generator does not have, and fails there.  `--datatype old` needs the actions_data_old
loader, which this project does not have, and is refused.
"""
import argparse
import os
import sys

import numpy as np


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m acimg.features", description=__doc__.split("\n")[0])
    ap.add_argument("--model", type=str, default="UNet", help="model type (UNet)")
    ap.add_argument("--train_file", type=str, required=True, help="text file listing the TFRecord files")
    ap.add_argument("--init_checkpoint", type=str, required=True, help="Saver-V2 checkpoint prefix (.../epoch_N.ckpt)")
    ap.add_argument("--encoder_type", type=str, default="Video", help="names the output directory")
    ap.add_argument("--batch_size", type=int, default=2)
    ap.add_argument("--num_skip_conn", type=int, default=1, choices=(0, 1, 2))
    ap.add_argument("--ae", type=int, default=0, help="1: plain auto-encoder generator (its code, no sampling)")
    ap.add_argument("--datatype", type=str, default="outdoor", help="outdoor or music ('old' is not supported)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the eps draws")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def dataset_name(args):
    return args.train_file.split("/")[-1].split(".")[0]


def output_dir(args):
    """<checkpoint dir>/<dataset>_<encoder_type>_<checkpoint number> (extract_features_unetraces.py:39-45)"""
    s = args.init_checkpoint.split("/")[-1]
    name = "{}_{}_{}".format(dataset_name(args), args.encoder_type, (s.split("_")[1]).split(".ckpt")[0])
    return "/".join(args.init_checkpoint.split("/")[:-1] + [name])


def output_files(args):
    d, ds = output_dir(args), dataset_name(args)
    return tuple("{}/{}_{}.npy".format(d, ds, kind) for kind in ("data", "labels", "scenario"))


def run(args, trainer=None, log=print):
    """extract and save; returns {'data', 'labels', 'scenario': the saved arrays, 'files': their paths}"""
    import torch

    from .data import TFRecordDataLoader
    from .localize import build_trainer
    from .unet_acresnet import Z
    if args.datatype == "old":
        raise ValueError("--datatype old needs the actions_data_old record loader, which is not supported")
    device = torch.device(args.device)
    tr = trainer if trainer is not None else build_trainer(args, device)
    data = TFRecordDataLoader(args.train_file, args.batch_size, device=device)
    gen = torch.Generator().manual_seed(int(args.seed))
    feats, labels, scen = [], [], []
    for batch in data.data:
        n = int(batch[1].reshape(-1, 12).shape[0])
        eps = torch.randn(n, Z, generator=gen)
        feats.append(tr.features(batch, eps=eps).double().cpu().numpy())
        labels.append(batch[3].reshape(n, -1).numpy())
        scen.append(batch[4].reshape(n, -1).numpy())
        log("{} samples".format(sum(len(f) for f in feats)))
    if not feats:
        raise ValueError("no samples in %s" % args.train_file)
    out = dict(data=np.concatenate(feats).astype(np.float64), labels=np.concatenate(labels).astype(int),
               scenario=np.concatenate(scen).astype(int))
    os.makedirs(output_dir(args), exist_ok=True)
    files = output_files(args)
    for f, key in zip(files, ("data", "labels", "scenario")):
        np.save(f, out[key])
    log("Completed, got {} samples".format(out["data"].shape[0]))
    out["files"] = files
    return out


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
