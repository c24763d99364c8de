"""`python -m acimg.main --mode train --model UNet --embedding 1 --mfcc 1` end to end on two 12-frame records: what it
writes (configuration.txt, checkpoints, ONE event file), what the event file holds (scalars, the eight images, the
variables' histograms, valid_loss) against the restatements of tests/summary_ref.py, that the pipelined and the
one-stream run write the same events, and that a run without a logger computes the same losses and writes no log."""
import glob
import io
import os
from collections import OrderedDict

import numpy as np
import pytest

import summary_ref as sref
from data_support import write_outdoor_records
from model_support import loss_lines

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    """three runs of the command line on the same records, unshuffled: no logger (one stream; its train_step is watched:
    first target frame, first generated frame and losses of every batch, the variables after the last), logger with
    histograms on one stream, the same pipelined"""
    from acimg.main import run_main
    tmp = tmp_path_factory.mktemp("cli")
    paths = write_outdoor_records(tmp, 23, [(3 + r, 5 + r) for r in range(2)], wide=True)
    train, valid = str(tmp / "train.txt"), str(tmp / "valid.txt")
    with open(train, "w") as f:
        f.write("\n".join(paths) + "\n")
    with open(valid, "w") as f:
        f.write(paths[0] + "\n")
    out = {}
    for name, pipeline, logged in (("off", 0, False), ("p0", 0, True), ("p1", 1, True)):
        log, seen, box = [], [], {}

        def hook(tr, seen=seen, box=box, watch=not logged):
            box["trainer"] = tr
            if watch:
                step = tr.train_step

                def watched(batch, **kw):
                    r = step(batch, **kw)
                    g = tr._graph_for(12)
                    seen.append((batch[0][0].cpu().numpy().copy(), g.modelac.output[0].cpu().numpy().copy(), r))
                    return r
                tr.train_step = watched

        t = [1000.0]

        def clock(t=t):
            t[0] += 0.5
            return t[0]

        argv = ["--mode", "train", "--model", "UNet", "--embedding", "1", "--mfcc", "1", "--batch_size", "12",
                "--num_epochs", "1", "--display_freq", "1", "--exp_name", name, "--train_file", train, "--valid_file", valid,
                "--checkpoint_dir", str(tmp / "ckpt"), "--pipeline", str(pipeline), "--device", str(device)]
        if logged:
            argv += ["--tensorboard", str(tmp / "tb"), "--histograms", "1"]
        best = run_main(argv, log=log.append, hooks=dict(shuffle=False, trainer=hook, logger=dict(clock=clock, hostname="h")))
        tr = box["trainer"]
        out[name] = dict(log=log, best=best, seen=seen, store=tr.session.store, steps=tr.global_step, train=train, valid=valid,
                         ckpt=str(tmp / "ckpt" / name), tb=str(tmp / "tb" / name))
        if not logged:
            out[name]["state"] = tr.session.store.state_dict()
            assert tr.logger is None and not os.path.exists(str(tmp / "tb"))      # no logger: no log
    return out


def _events(run):
    from acimg import events
    files = glob.glob(run["tb"] + "/events.out.tfevents.*")
    assert len(files) == 1, files
    assert os.path.basename(files[0]) == "events.out.tfevents.0000001000.h"
    return events.read_events(files[0])


@pytest.mark.parametrize("name", ["p0", "p1"])
def test_files(runs, name):
    run = runs[name]
    assert run["steps"] == 2 and np.isfinite(run["best"])
    assert open(run["ckpt"] + "/configuration.txt").read() == (
        "Experiment: {} \nModel: UNet \nLearning_rate: 0.001\n"
        "Num_epochs: 1 \nTotal_length: 30 \nSample_length: 1\n"
        "Number_of_crops: 30 \nMargin: 0.2\nNumber of classes: 10\n"
        "Block_size: 1 \nEmbedding: 1\nLatent weight: 1e-06\n"
        "Train_file: {} \nValid_file: {} \nTest_file: None\n"
        "Mode: train \nVisual_init_checkpoint: None \nAcoustic_init_checkpoint: None \nRestore_checkpoint: None\n"
        "Checkpoint_dir: {} \nLog dir: {} \nBatch_size: 12\n"
        "Number of skip connections: 1 \nAuto encoder: 0\nHuber: 1\nMSE: 1\n").format(
            name, run["train"], run["valid"], os.path.dirname(run["ckpt"]), os.path.dirname(run["tb"]))
    for f in ("epoch_random.ckpt.index", "epoch_0.ckpt.index", "epoch_0.ckpt.data-00000-of-00001", "model.txt", "checkpoint"):
        assert os.path.exists(run["ckpt"] + "/" + f), f
    ev = _events(run)
    assert ev[0]["file_version"] == "brain.Event:2" and "summary" not in ev[0]
    assert [e["step"] for e in ev] == [0, 1, 2, 0]


@pytest.mark.parametrize("name", ["p0", "p1"])
def test_scalars_and_images(runs, name):
    from PIL import Image
    ev = _events(runs[name])
    seen = runs["off"]["seen"]
    assert len(seen) == 2
    for k, e in enumerate(ev[1:3]):
        target, generated, losses = seen[k]
        vals = OrderedDict((v["tag"], v) for v in e["summary"])
        tags = list(vals)
        assert tags[:4] == ["l2_loss", "l1_loss", "train_loss", "latent_loss"]
        assert tags[4:12] == ["mfcc%d/image" % i for i in range(4)] + ["reconstructed%d/image" % i for i in range(4)]
        for tag, key in (("l2_loss", "mse"), ("l1_loss", "huber"), ("train_loss", "loss"), ("latent_loss", "latent")):
            assert vals[tag]["simple_value"] == float(np.float32(losses[key])), (k, tag)
        for i in range(4):
            for tag, src in (("mfcc%d/image" % i, target), ("reconstructed%d/image" % i, generated)):
                im = vals[tag]["image"]
                assert (im["height"], im["width"], im["colorspace"]) == (36, 48, 3)
                px = np.asarray(Image.open(io.BytesIO(im["encoded_image_string"])).convert("RGB"))
                want = sref.normalize_image(src[:, :, 3 * i:3 * i + 3])
                assert np.array_equal(px, want), (k, tag, int((px != want).sum()))
        assert len(set(bytes(vals["reconstructed%d/image" % i]["image"]["encoded_image_string"]) for i in range(4))) == 4
    (v,) = ev[3]["summary"]
    assert v["tag"] == "valid_loss" and v["simple_value"] == float(np.float32(runs[name]["best"]))


def test_pipeline_is_a_pure_schedule(runs):
    a, b = _events(runs["p0"]), _events(runs["p1"])
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x["step"] == y["step"]
        assert x.get("summary") == y.get("summary")          # tags, order, scalars, PNG bytes, histograms
    assert loss_lines(runs["p0"]["log"], validation=True) == loss_lines(runs["p1"]["log"], validation=True)


def test_histograms(runs):
    from acimg import events
    run = runs["p1"]
    store, state = runs["off"]["store"], runs["off"]["state"]
    names = [n for n in store.tf_names() if n in store.grad_dict()]
    assert len(names) > 20 and any("/mean/kernel" in n for n in names) and any("/std/bias" in n for n in names)
    limits = events.default_bucket_limits()
    ev = _events(run)
    for e in ev[1:3]:
        hist = OrderedDict((v["tag"], v["histo"]) for v in e["summary"] if "histo" in v)
        assert list(hist) == [events.sanitize_tag(n + ":0") for n in names]
        for n in names:
            assert hist[events.sanitize_tag(n + ":0")]["num"] == float(np.prod(state[n].shape)), n
    hist = OrderedDict((v["tag"], v["histo"]) for v in ev[2]["summary"] if "histo" in v)      # after the last update
    for n in names:
        h = hist[events.sanitize_tag(n + ":0")]
        counts, stats, bad = sref.histogram(state[n].numpy(), limits)
        assert bad == 0
        assert (h["bucket_limit"], h["bucket"]) == sref.compress(counts, limits), n
        assert h["min"] == stats["min"] and h["max"] == stats["max"], n
        d = state[n].numpy().astype(np.float64).reshape(-1)
        assert abs(h["sum"] - stats["sum"]) <= d.size * 2.0 ** -53 * np.abs(d).sum(), n
        assert abs(h["sum_squares"] - stats["sum_squares"]) <= d.size * 2.0 ** -53 * (d * d).sum(), n


def test_logger_off_changes_nothing(runs):
    off, on = runs["off"], runs["p0"]
    lines = loss_lines(off["log"], validation=True)
    assert len(lines) == 3 and lines == loss_lines(on["log"], validation=True)
    assert off["best"] == on["best"] and off["steps"] == on["steps"] == 2
    assert not glob.glob(off["ckpt"] + "/events*")
    a = off["state"]
    b = on["store"].state_dict()
    assert list(a) == list(b)
    for n in a:
        assert a[n].numpy().tobytes() == b[n].numpy().tobytes(), n          # the variables too: bit-equal
