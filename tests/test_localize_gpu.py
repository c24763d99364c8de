"""Localisation evaluation on the device: `acimg_box_iou` against the NumPy restatement of showimages_bb.py:286-320
(exact half-unit counts, the resized mask, the IoU, NaN for 0 / 0, the exact-tie columns 74 and 223), and end to end:
`Trainer.generate`, `python -m acimg.localize` on box-annotated records (the box metric) and on `TFRecordDataLoader`
records (the energy metric), with the reference's accuracy files and the area under the curve."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import localize_ref as ref  # noqa: E402
from data_support import outdoor_record, random_box_record  # noqa: E402
from localize_ref import random_boxes  # noqa: E402

pytestmark = pytest.mark.gpu


def run_box_iou(device, logen, boxes):
    from acimg import ops
    N = logen.shape[0]
    plan = ops.Plan(device, eager=True)
    lg = torch.from_numpy(np.ascontiguousarray(logen, np.float32).reshape(N, 36 * 48)).to(device)
    bx = torch.from_numpy(np.ascontiguousarray(boxes, np.int32).reshape(N, 4, 3)).to(device)
    iou = torch.empty(N, dtype=torch.float32, device=device)
    counts = torch.full((N, 2), -7, dtype=torch.int32, device=device)
    mask = torch.full((N, 224, 298), 9, dtype=torch.uint8, device=device)
    ops.box_iou(plan, lg, bx, N, iou, counts, mask)
    iou2 = torch.empty(N, dtype=torch.float32, device=device)
    ops.box_iou(plan, lg, bx, N, iou2)                   # optional outputs omitted: same IoU
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(iou.cpu().numpy(), iou2.cpu().numpy())
    return iou.cpu().numpy(), counts.cpu().numpy(), mask.cpu().numpy()


def check_against_restatement(device, logen, boxes):
    iou, counts, mask = run_box_iou(device, logen, boxes)
    for n in range(logen.shape[0]):
        num, den, want, m2 = ref.box_iou(logen[n], boxes[n])
        assert (counts[n, 0], counts[n, 1]) == (num, den), n
        assert np.array_equal(mask[n], m2.astype(np.uint8)), n
        if den == 0:
            assert np.isnan(iou[n]) and np.isnan(want), n
        else:
            assert abs(float(iou[n]) - want) <= 1e-7 * max(abs(want), 1e-30), (n, iou[n], want)
    return iou, counts, mask


@pytest.mark.parametrize("N", [1, 7, 64, 257])
def test_box_iou_matches_restatement_random(device, N):
    """N = 257: box_iou_finish_kernel takes one workgroup per 256 samples, so a second workgroup with one sample"""
    rng = np.random.RandomState(N)
    logen = (rng.rand(N, 36, 48) * rng.rand(N, 1, 1) * 3).astype(np.float32)
    check_against_restatement(device, logen, random_boxes(rng, N))


def test_box_iou_tie_columns_and_nan(device):
    rng = np.random.RandomState(11)
    maps, boxes = [], []
    for edge in (12, 36):                                # mask edges land on output columns 74 and 223 (f = 0.5)
        for rows in (slice(0, 36), slice(0, 10), slice(7, 29), slice(20, 36)):
            m = np.full((36, 48), 0.25, np.float32)
            m[rows, :edge] = 1.0
            maps.append(m)
            maps.append(m[:, ::-1].copy())               # the same edge from the other side (columns 11 | 12 mirrored)
    maps = np.stack(maps)
    boxes = random_boxes(rng, maps.shape[0])
    iou, counts, mask = check_against_restatement(device, maps, boxes)
    m12 = mask[0]
    assert m12[:, 74].sum() == 2 and m12[:, :74].all() and not m12[:, 75:].any()
    m36 = mask[8]
    assert m36[:, 223].sum() == 2 and m36[:, :223].all() and not m36[:, 224:].any()
    # empty mask (constant map: nothing above its mean) and no box: 0 / 0 = NaN; with a box: IoU 0
    const = np.full((2, 36, 48), 0.3, np.float32)
    b = np.zeros((2, 4, 3), np.int32)
    b[1, :, 0] = (5, 20, 5, 20)
    iou, counts, mask = check_against_restatement(device, const, b)
    assert np.isnan(iou[0]) and tuple(counts[0]) == (0, 0) and iou[1] == 0.0 and not mask.any()


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_generate_and_localize_end_to_end(device, tmp_path):
    from acimg import localize, tfio
    from acimg.data import BoxRecordLoader, TFRecordDataLoader
    from acimg.evaluate import EnergyIoU, accuracy_curve, area_under_curve
    from acimg.flags import FLAGS
    from acimg.frontend import FrontEnd
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc, Z
    from acimg.vision import ResNet50Model

    rng = np.random.RandomState(21)
    # a "trained" generator: random variables with non-trivial moving statistics, saved as a Saver-V2 bundle
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    src = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                  ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    src._build_functions(batch_size=2)
    src.modelimages.initialize()
    src.modelac.initialize()
    state = OrderedDict((k, v.numpy()) for k, v in src.session.store.state_dict().items())
    for k in state:
        if k.endswith("/moving_mean"):
            state[k] = (rng.randn(*state[k].shape) * 0.05).astype(np.float32)
        elif k.endswith("/moving_variance"):
            state[k] = rng.uniform(0.5, 2.0, size=state[k].shape).astype(np.float32)
    ckdir = tmp_path / "ckpt"
    ckdir.mkdir()
    ckpt = str(ckdir / "epoch_7.ckpt")
    tfio.write_checkpoint(ckpt, state)

    files = [str(tmp_path / "f0.tfrecord"), str(tmp_path / "f1.tfrecord")]
    tfio.write_tfrecord(files[0], [random_box_record(rng, 12288), random_box_record(rng, 24576)], compression="GZIP")
    tfio.write_tfrecord(files[1], [random_box_record(rng, 15001)], compression="GZIP")
    listing = tmp_path / "flickr_test.txt"
    listing.write_text("\n".join(files) + "\n")

    args = localize.parse_args(["--model", "UNet", "--train_file", str(listing), "--init_checkpoint", ckpt,
                                "--batch_size", "2", "--num_skip_conn", "1", "--ae", "0", "--threshold", "0.5",
                                "--datatype", "flickr"])
    tr = localize.build_trainer(args, device)
    # Trainer.generate == eval_step's generator output, full and partial batch (same noise)
    for b in BoxRecordLoader(str(listing), 2).data:
        n = b[1].shape[0]
        eps = torch.randn(n, Z, generator=torch.Generator().manual_seed(n))
        got = tr.generate(b, eps=eps).clone()
        assert got.shape == (n, 36, 48, 12)
        tr.eval_step(b, eps=eps)
        assert torch.equal(got, tr._graph_for(n).modelac.output)
        assert torch.isfinite(got).all() and float(got.std()) > 0

    res = localize.run(args, trainer=tr, keep_generated=True, log=lambda *a: None)
    gen = res["generated"]
    assert gen.shape == (3, 36, 48, 12) and res["num_samples"] == 3
    fe = FrontEnd(device)
    logen = fe.find_logen(torch.from_numpy(gen).to(device)).cpu().numpy().reshape(3, 36, 48)
    boxes = np.concatenate([torch.stack(list(b[3:7]), 1).numpy() for b in BoxRecordLoader(str(listing), 2).data])
    want = [ref.box_iou(logen[n], boxes[n])[2] for n in range(3)]
    got = [float("nan") if v is None else v for v in res["iou"]]
    np.testing.assert_array_equal(np.array(got), np.array(want))
    acc = accuracy_curve(want)
    d = localize.output_dir(args)
    assert d.endswith("/ckpt/UNet_flickr_test_AcousticFramesJet2_7")
    with open(localize.accuracy_file(d, 0.5)) as f:
        assert f.read() == "iou {:6f}".format(acc[5])
    with open(os.path.join(d, localize.RESULT_FILE)) as f:
        js = json.load(f)
    assert js["accuracy"] == list(acc) and js["auc"] == area_under_curve(acc) and js["metric"] == "box"

    # the energy path on TFRecordDataLoader records: the same curve as EnergyIoU applied batch by batch
    ofiles = [str(tmp_path / "o0.tfrecord"), str(tmp_path / "o1.tfrecord")]
    tfio.write_tfrecord(ofiles[0], [outdoor_record(rng, 2, 7, wide=False)], compression="GZIP")
    tfio.write_tfrecord(ofiles[1], [outdoor_record(rng, 4, 7, wide=False)], compression="GZIP")
    olist = tmp_path / "testing.txt"
    olist.write_text("\n".join(ofiles) + "\n")
    oargs = localize.parse_args(["--train_file", str(olist), "--init_checkpoint", ckpt, "--batch_size", "2",
                                 "--datatype", "outdoor", "--ae", "0"])
    ores = localize.run(oargs, trainer=tr, keep_generated=True, log=lambda *a: None)
    ogen = ores["generated"]
    assert ogen.shape == (24, 36, 48, 12)
    metric = EnergyIoU(device)
    real = torch.cat([b[0] for b in TFRecordDataLoader(str(olist), 2, device=device).data])
    ious = []
    for i in range(0, 24, 2):
        ious.append(metric.iou(real[i:i + 2].to(device), torch.from_numpy(ogen[i:i + 2]).to(device)).cpu().numpy())
    ious = np.concatenate(ious).astype(np.float64)
    np.testing.assert_array_equal(np.array(ores["iou"], np.float64), ious)
    assert ores["accuracy"] == list(accuracy_curve(ious)) and ores["metric"] == "energy"
    od = localize.output_dir(oargs)
    assert od.endswith("/ckpt/UNet_testing_Acoustictry_7")
    for t, a in zip(ores["thresholds"], ores["accuracy"]):
        with open(localize.accuracy_file(od, t)) as f:
            assert f.read() == "iou {:6f}".format(a)
