"""`python -m acimg.main`: the reference's main.py - its flags, its dispatch - for the generator's training run.

    python -m acimg.main --mode train --model UNet --embedding 1 --mfcc 1 --exp_name E --train_file T --valid_file V \\
        --checkpoint_dir C --tensorboard B [--num_skip_conn 1 --ae 0 --batch_size 32 --num_epochs 300 ...]

builds what main.py:203-229 builds for `--embedding 1 --mfcc 1` (ResNet50Model + UNetAc(num_skip_conn) + the trainer of
trainer/mfcctrainer.py), writes `configuration.txt` (main.py:247-276, the embedding branch), trains with the
`epoch_<n>.ckpt` bundles and `model.txt`, and - when `--tensorboard` is given - logs to `<tensorboard>/<exp_name>` what
the reference logs: scalars and the eight image summaries on every displayed step, `valid_loss` per epoch
(`--histograms 1`: also one histogram per trainable variable).  `--mode test` scores `--test_file`.

`--correspondence 1` (the published recipe, scripts/scriptacresn.bash) reaches the three loaders: every frame a second
time with the MFCC of its low-passed sound, tiled, as the target (dataloader/outdoor_data_mfcc.py:108-113); the
training loader, the one that shuffles, also runs the second shuffle stage, validation and test see batches of
2 * batch_size rows.

`--embedding 0 --model DualCamNet` is the classification experiment: `classify.run_main`.  Every other branch of
main.py's dispatch names a trainer whose step this project has as a class without main.py's loop around it, or does not
have: they are refused with that name.  Extras beside main.py's flags: `--device`, `--seed` (the eps draws),
`--histograms`.  Records come through `DeviceDataLoader`; one GPU.
"""
import argparse
import os
import sys
from datetime import datetime

from .classify import refuse_old

NUM_CLASSES = 10        # main.py:139, datatype outdoor


def dispatch(flags):
    """main.py:175-240,286-323 as a pure function of the flags: the route, one of
         "generator"  --embedding 1 --mfcc 1 (proxy, project, jointmvae 0): this module's run
         "classify"   --embedding 0 --model DualCamNet: classify.run_main
       ValueError for every other branch, naming what main.py would build there."""
    f = flags
    if f.embedding:
        if f.proxy:
            raise ValueError("--proxy 1 is TrainerNCAproxyanchor, which is not built")
        if f.project:
            raise ValueError("--project 1 is TrainerProject: its step is acimg.trainer_associator.TrainerAssociator, a class "
                             "without main.py's loop; there is no command line for it")
        if f.jointmvae:
            raise ValueError("--jointmvae 1 is TrainerMulti: its step is acimg.trainer_multi.TrainerMulti, a class without "
                             "main.py's loop; there is no command line for it")
        if f.mfcc:
            return "generator"
        raise ValueError("--embedding 1 --mfcc 0 is TrainerLoss, which is not built")
    if f.model == "UNet":
        raise ValueError("--embedding 0 --model UNet is the single-modality VAE: its step is acimg.trainer_vae.TrainerVAE, a "
                         "class without main.py's loop; there is no command line for it")
    if f.model == "DualCamNet":
        if f.correspondence:
            raise ValueError("--correspondence 1 with --embedding 0: the pair map tiles reshape(-1, 1, 12) of a clip batch, "
                             "which has no defined meaning for the classification experiment's clips")
        return "classify"
    raise ValueError("Unknown model type %r" % (f.model,))


def configuration_text(flags, num_classes=NUM_CLASSES):
    """main.py:247-276: configuration.txt of the embedding branch"""
    f = flags
    return ('Experiment: {} \nModel: {} \nLearning_rate: {}\n'.format(f.exp_name, f.model, f.learning_rate)
            + 'Num_epochs: {} \nTotal_length: {} \nSample_length: {}\n'.format(f.num_epochs, f.total_length,
                                                                             f.sample_length)
            + 'Number_of_crops: {} \nMargin: {}\nNumber of classes: {}\n'.format(f.number_of_crops, f.margin, num_classes)
            + 'Block_size: {} \nEmbedding: {}\nLatent weight: {}\n'.format(f.block_size, f.embedding, f.latent_loss)
            + 'Train_file: {} \nValid_file: {} \nTest_file: {}\n'.format(f.train_file, f.valid_file, f.test_file)
            + 'Mode: {} \nVisual_init_checkpoint: {} \nAcoustic_init_checkpoint: {} \nRestore_checkpoint: {}\n'.format(
                f.mode, f.visual_init_checkpoint, f.acoustic_init_checkpoint, f.restore_checkpoint)
            + 'Checkpoint_dir: {} \nLog dir: {} \nBatch_size: {}\n'.format(f.checkpoint_dir, f.tensorboard, f.batch_size)
            + 'Number of skip connections: {} \nAuto encoder: {}\nHuber: {}\nMSE: {}\n'.format(f.num_skip_conn, f.ae,
                                                                                             f.huber_loss, f.MSE))


def parse(argv):
    """FLAGS.parse + this module's extras; the refusals that need no device"""
    from .flags import FLAGS
    rest = FLAGS.parse(argv)
    ap = argparse.ArgumentParser(prog="python -m acimg.main")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--histograms", type=int, default=0)
    ap.add_argument("--inflate", choices=["zlib", "device"], default="zlib",
                    help="who inflates the GZIP records: the loader's worker threads (zlib) or the device (acimg.inflate)")
    extra = ap.parse_args(rest)
    for name in ("mode", "exp_name"):          # flags.mark_flags_as_required(['mode', 'exp_name']), main.py:366
        if getattr(FLAGS, name) is None:
            raise ValueError("Flag --%s must have a value other than None." % name)
    if FLAGS.mode not in ("train", "test"):
        raise ValueError("Unknown execution mode")
    refuse_old(FLAGS.datatype)
    return FLAGS, extra


def build_trainer(device):
    """what main.py:203-229 builds for --embedding 1 --mfcc 1 from FLAGS"""
    from .flags import FLAGS
    from .session import Session
    from .trainer import Trainer
    from .unet_acresnet import UNetAc
    from .vision import ResNet50Model
    nr_frames = FLAGS.block_size * FLAGS.sample_length
    mi = ResNet50Model(input_shape=[224, 298, 3], num_classes=None)
    ma = UNetAc(input_shape=[36, 48, 12], embedding=FLAGS.ae, num_skip=FLAGS.num_skip_conn)
    return Trainer(ma, mi, display_freq=FLAGS.display_freq, learning_rate=FLAGS.learning_rate, num_classes=NUM_CLASSES,
                   num_epochs=FLAGS.num_epochs, temporal_pooling=FLAGS.temporal_pooling, nr_frames=nr_frames,
                   session=Session(device))


def run_main(argv, log=print, hooks=None):
    """main.py's main(): parse, dispatch, build, run.  hooks (tests): {"shuffle": bool} overrides the training loader's
    shuffle, {"logger": kwargs} reaches the Logger (clock, hostname), {"trainer": fn} sees the trainer before it runs."""
    hooks = hooks or {}
    FLAGS, extra = parse(argv)
    route = dispatch(FLAGS)
    if route == "classify":
        from . import classify
        rest = [a for a in argv]
        for i in range(len(rest) - 1, -1, -1):      # --histograms and --inflate are this module's own
            if rest[i] in ("--histograms", "--inflate"):
                del rest[i:i + 2]
            elif rest[i].startswith(("--histograms=", "--inflate=")):
                del rest[i]
        return classify.run_main(rest, log=log)
    import torch

    from . import dp
    from .data import DeviceDataLoader
    from .logger import Logger
    device = torch.device(extra.device)
    log('{}: {} - Creating data loaders'.format(datetime.now(), FLAGS.exp_name))

    def loader(files, shuffle):
        if files is None:
            return None
        return DeviceDataLoader(files, FLAGS.batch_size, shuffle=shuffle, buffer_size=FLAGS.buffer_size if shuffle else None,
                                embedding=FLAGS.embedding, num_actions=NUM_CLASSES, device=device,
                                correspondence=FLAGS.correspondence, inflate=extra.inflate)

    log('{}: {} - Building model'.format(datetime.now(), FLAGS.exp_name))
    log('{}: {} - Building trainer'.format(datetime.now(), FLAGS.exp_name))
    trainer = build_trainer(device)
    trainer.log = log
    if extra.seed is not None:
        trainer.noise_seed = int(extra.seed)
    if hooks.get("trainer") is not None:
        hooks["trainer"](trainer)
    if FLAGS.mode == "train":
        checkpoint_dir = '{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name)
        os.makedirs(checkpoint_dir, exist_ok=True)
        with open(checkpoint_dir + "/configuration.txt", "w") as outfile:
            outfile.write(configuration_text(FLAGS))
        if FLAGS.tensorboard is not None and dp.is_writer(trainer.group):
            trainer.logger = Logger('{}/{}'.format(FLAGS.tensorboard, FLAGS.exp_name), **hooks.get("logger", {}))
            trainer.log_histograms = bool(extra.histograms)
        log('{}: {} - Training started'.format(datetime.now(), FLAGS.exp_name))
        train_data = loader(FLAGS.train_file, hooks.get("shuffle", True))
        valid_data = loader(FLAGS.valid_file, False)
        try:
            return trainer.train(train_data=train_data, valid_data=valid_data)
        finally:
            for d in (train_data, valid_data):
                if d is not None:
                    d.close()
            if trainer.logger is not None:
                trainer.logger.close()
    log('{}: {} - Testing started'.format(datetime.now(), FLAGS.exp_name))
    test_data = loader(FLAGS.test_file, False)
    try:
        return trainer.test(test_data=test_data)
    finally:
        if test_data is not None:
            test_data.close()


def main(argv=None):
    run_main(sys.argv[1:] if argv is None else list(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
