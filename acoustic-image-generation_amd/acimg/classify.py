"""The classification experiment: `python -m acimg.classify --mode train | test | compare`.

`--mode train | test` stand where the reference's main.py stands for `--model DualCamNet` (main.py:297-362), with its
flags: DualCamNet trained / scored on generated acoustic images (ResNet50Model + UNetAc(num_skip) from
`--init_checkpoint`, in inference mode), or - `--mfcc 1` - on the real acoustic images, or - `--mfcc 1 --mfccmap 1` - on
the tiled MFCC map.  Training writes `configuration.txt` (:329-353), the `epoch_<n>.ckpt` bundles and `model.txt`;
testing writes `test_accuracy.txt` / `test_accuracy_<tag>.txt` / `test_accuracy_mfccmap_<tag>.txt` (`TrainerClass`).
Records come through `DeviceDataLoader(embedding=0)`: whole clips, shuffled with `--buffer_size` for training.

`--mode compare` stands where saveimagesresnet.py stands, with its flags (+ `--seed` for the generator's eps): ONE
DualCamNet restored from `--ac_checkpoint` scores the real clips of `--train_file` and then the generated clips of the
same records (trunk and generator from `--init_checkpoint`, inference mode), or the MFCC map under `--mfccmap 1`.
It writes `acc rec {} acc ac {}` to the file the script names (:212-217),

    <generator checkpoint dir>/test_unet<name>_dualcamnet<nameac>.txt        (--mfccmap 0)
    <classifier checkpoint dir>/test_map_dualcamnet<nameac>.txt              (--mfccmap 1)

and beside it `classification.json`: both confusion matrices (row = label, column = prediction), per-class recall
(null for a class with no clip), losses, clip counts and the number of clips whose label was out of range.  The
accuracies are ratios of the integer counts of `acimg_clip_eval`.  `--datatype old` needs the actions_data_old
loader, which this project does not have, and is refused in every mode.
"""
import argparse
import json
import os
import sys
from datetime import datetime

MODES = ("train", "test", "compare")


def build_compare_parser():
    ap = argparse.ArgumentParser(prog="python -m acimg.classify --mode compare", description=__doc__.split("\n")[0])
    ap.add_argument("--mode", type=str, default="compare")
    ap.add_argument("--train_file", type=str, required=True, help="text file listing the TFRecord files")
    ap.add_argument("--init_checkpoint", type=str, default=None, help="generator checkpoint prefix (.../epoch_N.ckpt)")
    ap.add_argument("--ac_checkpoint", type=str, required=True, help="DualCamNet checkpoint prefix (.../epoch_N.ckpt)")
    ap.add_argument("--batch_size", type=int, default=16, help="clips per batch")
    ap.add_argument("--sample_length", type=int, default=1)
    ap.add_argument("--mfccmap", type=int, default=0, help="1: score the tiled MFCC map instead of generated images")
    ap.add_argument("--datatype", type=str, default="outdoor", help="outdoor or music ('old' is not supported)")
    ap.add_argument("--num_skip_conn", type=int, default=1, choices=(0, 1, 2))
    ap.add_argument("--ae", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0, help="seed of the generator's eps draws")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def mode_of(argv):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--mode", type=str, default=None)
    mode = ap.parse_known_args(argv)[0].mode
    if mode not in MODES:
        raise ValueError("Unknown execution mode %r (--mode is one of %s)" % (mode, ", ".join(MODES)))
    return mode


def refuse_old(datatype):
    if datatype == "old":
        raise ValueError("--datatype old needs the actions_data_old record loader, which is not supported")


def checkpoint_number(checkpoint):
    """'<dir>/epoch_12.ckpt' -> '12' (saveimagesresnet.py:37-40)"""
    s = checkpoint.split("/")[-1]
    return (s.split("_")[1]).split(".ckpt")[0]


def compare_file(args):
    """the text file saveimagesresnet.py:212-217 writes"""
    nameac = checkpoint_number(args.ac_checkpoint)
    if int(args.mfccmap) == 0:
        if args.init_checkpoint is None:
            raise ValueError("--init_checkpoint (the generator) is needed unless --mfccmap 1")
        return "{}".format(str.join("/", args.init_checkpoint.split("/")[:-1])) + "/test_unet{}_dualcamnet{}.txt".format(
            checkpoint_number(args.init_checkpoint), nameac)
    return "{}".format(str.join("/", args.ac_checkpoint.split("/")[:-1])) + "/test_map_dualcamnet{}.txt".format(nameac)


def compare_json_file(args):
    return "/".join(compare_file(args).split("/")[:-1] + ["classification.json"])


def recall(confusion):
    """per-class recall from a confusion matrix (row = label): None for a class with no clip"""
    out = []
    for k, row in enumerate(confusion):
        n = int(sum(int(v) for v in row))
        out.append(int(row[k]) / n if n else None)
    return out


def summary(result):
    """the JSON form of a `ClipEvaluator.result()`"""
    conf = [[int(v) for v in row] for row in result["confusion"]]
    clips = int(result["clips"])
    return dict(loss=float(result["loss"]) if clips else None, accuracy=int(result["correct"]) / clips if clips else None,
                clips=clips, correct=int(result["correct"]), invalid=int(result["invalid"]), confusion=conf,
                recall=recall(conf))


def compare_document(args, ac, rec, num_classes):
    """classification.json: `ac` / `rec` are the two `ClipEvaluator.result()`s"""
    return dict(train_file=args.train_file, init_checkpoint=args.init_checkpoint, ac_checkpoint=args.ac_checkpoint,
                mfccmap=int(args.mfccmap), seed=int(args.seed), batch_size=int(args.batch_size),
                num_classes=int(num_classes), scored="mfccmap" if int(args.mfccmap) else "generated",
                ac=summary(ac), rec=summary(rec))


def _classifier(num_classes):
    from .dualcamnet import DualCamHybridModel
    return DualCamHybridModel(input_shape=[36, 48, 12], num_classes=num_classes, embedding=0)


def _generator(num_skip, ae):
    from .unet_acresnet import UNetAc
    from .vision import ResNet50Model
    return (ResNet50Model(input_shape=[224, 298, 3], num_classes=None),
            UNetAc(input_shape=[36, 48, 12], embedding=bool(ae), num_skip=int(num_skip)))


def run_compare(args, log=print):
    """score and write both files; returns the document of classification.json (+ 'files')"""
    import torch

    from .data import DeviceDataLoader
    from .flags import FLAGS
    from .session import Session
    from .trainer_class import TrainerClass
    refuse_old(args.datatype)
    txt, js = compare_file(args), compare_json_file(args)
    device = torch.device(args.device)
    num_classes = 10
    FLAGS.model, FLAGS.ae, FLAGS.num_skip_conn = "DualCamNet", int(args.ae), int(args.num_skip_conn)
    log('{} - Creating data loaders'.format(datetime.now()))
    data = DeviceDataLoader(args.train_file, args.batch_size, shuffle=False, embedding=0, num_actions=num_classes,
                            device=device)
    log('{} - Building model'.format(datetime.now()))
    frames = int(args.batch_size) * 12
    real = TrainerClass(_classifier(num_classes), None, None, num_classes=num_classes, session=Session(device),
                        source="acoustic")
    real._build_functions(batch_size=frames)
    if int(args.mfccmap):
        other = TrainerClass(_classifier(num_classes), None, None, num_classes=num_classes, session=Session(device),
                             source="mfccmap")
    else:
        mi, ma = _generator(args.num_skip_conn, args.ae)
        other = TrainerClass(_classifier(num_classes), mi, ma, num_classes=num_classes, session=Session(device),
                             source="generated")
        other.noise_seed = int(args.seed)
    other._build_functions(batch_size=frames)
    log('{} - Restoring student model'.format(datetime.now()))
    for tr in (real, other):
        tr.log = lambda *a: None
        tr._initialize()
        tr._load(args.ac_checkpoint, [tr.model])
    if not int(args.mfccmap):
        other._load(args.init_checkpoint, [other.model_encoder_images, other.model_encoder_acoustic])
    log('{} - Done'.format(datetime.now()))
    real._begin_pass()
    other._begin_pass()
    total = 0
    try:
        for next_batch in data.data:
            real._pass_batch(next_batch)
            other._pass_batch(next_batch)
            total += int(next_batch[3].shape[0])
            log(total)
    finally:
        data.close()
    ac, rec = real._end_pass(), other._end_pass()
    if not ac["clips"]:
        raise ValueError("no clip with a known class in %s" % args.train_file)
    log('{} - Completed, got {} samples'.format(datetime.now(), total))
    acctot, accrectot = ac["correct"] / ac["clips"], rec["correct"] / rec["clips"]
    line = 'acc rec {} acc ac {}'.format(accrectot, acctot)
    log(line)
    with open(txt, "w") as outfile:
        outfile.write(line)
    doc = compare_document(args, ac, rec, num_classes)
    with open(js, "w") as outfile:
        json.dump(doc, outfile, indent=1)
        outfile.write("\n")
    doc["files"] = (txt, js)
    return doc


def configuration_text(flags, num_classes):
    """main.py:329-353"""
    f = flags
    return ('Experiment: {} \nBatch_size: {}\n Latent weight: {}\n'.format(f.exp_name, f.batch_size, f.latent_loss)
            + 'Model: {} \nLearning_rate: {}\nNumber of classes: {}\n'.format(f.model, f.learning_rate, num_classes)
            + 'Num_epochs: {} \nTotal_length: {} \nSample_length: {}\n'.format(f.num_epochs, f.total_length,
                                                                             f.sample_length)
            + 'Number_of_crops: {} \nCheckpoint_dir: {} \nLog dir: {}\n'.format(f.number_of_crops, f.checkpoint_dir,
                                                                              f.tensorboard)
            + 'Train_file: {} \nValid_file: {} \nTest_file: {}\n'.format(f.train_file, f.valid_file, f.test_file)
            + 'Number of skip connections: {} \nAuto encoder: {}\nHuber: {}\nMSE: {}\n'.format(f.num_skip_conn, f.ae,
                                                                                             f.huber_loss, f.MSE)
            + 'Mode: {} \nInit_checkpoint: {} \nRestore_checkpoint: {}\n'.format(f.mode, f.init_checkpoint,
                                                                               f.restore_checkpoint))


def build_trainer(device, num_classes=10):
    """the trainer main.py:297-323 builds for `--model DualCamNet` from FLAGS"""
    from .flags import FLAGS
    from .session import Session
    from .trainer_class import TrainerClass
    nr_frames = 12 * FLAGS.sample_length
    mi, ma = (None, None) if FLAGS.mfcc else _generator(FLAGS.num_skip_conn, FLAGS.ae)
    return TrainerClass(_classifier(num_classes), mi, ma, display_freq=FLAGS.display_freq,
                        learning_rate=FLAGS.learning_rate, num_classes=num_classes, num_epochs=FLAGS.num_epochs,
                        temporal_pooling=FLAGS.temporal_pooling, nr_frames=nr_frames, session=Session(device))


def run_main(argv, log=print):
    """--mode train | test with main.py's flags (+ --device, --seed: the eps draws of the generated source)"""
    import torch

    from .data import DeviceDataLoader
    from .flags import FLAGS
    rest = FLAGS.parse(argv)
    ap = argparse.ArgumentParser(prog="python -m acimg.classify")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--seed", type=int, default=None)
    extra = ap.parse_args(rest)
    refuse_old(FLAGS.datatype)
    if FLAGS.model != "DualCamNet":
        raise ValueError("Unknown model type %r (python -m acimg.classify runs --model DualCamNet)" % FLAGS.model)
    if FLAGS.sample_length != 1:
        raise ValueError("--sample_length %d: the records hold one second, 12 frames" % FLAGS.sample_length)
    device = torch.device(extra.device)
    num_classes = 10
    log('{}: {} - Creating data loaders'.format(datetime.now(), FLAGS.exp_name))

    def loader(files, shuffle):
        if files is None:
            return None
        return DeviceDataLoader(files, FLAGS.batch_size, shuffle=shuffle, buffer_size=FLAGS.buffer_size, embedding=0,
                                num_actions=num_classes, device=device)

    log('{}: {} - Building trainer'.format(datetime.now(), FLAGS.exp_name))
    trainer = build_trainer(device, num_classes)
    trainer.log = log
    if extra.seed is not None:
        trainer.noise_seed = int(extra.seed)
    if FLAGS.mode == "train":
        checkpoint_dir = '{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name)
        os.makedirs(checkpoint_dir, exist_ok=True)
        with open(checkpoint_dir + "/configuration.txt", "w") as outfile:
            outfile.write(configuration_text(FLAGS, num_classes))
        log('{}: {} - Training started'.format(datetime.now(), FLAGS.exp_name))
        return trainer.train(train_data=loader(FLAGS.train_file, True), valid_data=loader(FLAGS.valid_file, False))
    log('{}: {} - Testing started'.format(datetime.now(), FLAGS.exp_name))
    return trainer.test(test_data=loader(FLAGS.test_file, False))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if mode_of(argv) == "compare":
        run_compare(build_compare_parser().parse_args(argv))
    else:
        run_main(argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
