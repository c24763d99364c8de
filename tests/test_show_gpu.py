"""Localisation overlays on the device: `acimg_overlay_render` against the NumPy restatement of its rule
(tests/render_ref.py) byte for byte - no tolerance, no pixel left out - over batch sizes, strides, a two-panel canvas
inside guard bands, boxes, replay, degenerate samples and foreign tables; and `python -m acimg.show` end to end on
records written here: every PNG decodes to the restatement applied to that frame and to the device's energy map."""
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

import render_ref as ref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402
from data_support import outdoor_record, random_box_record  # noqa: E402
from localize_ref import random_boxes  # noqa: E402
from render_ref import read_png  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "render_golden.npz"))
JET, GRAY = GOLD["table_jet"], GOLD["table_gray"]
H, W = 224, 298


def device_render(device, frames, logen, boxes=None, base=GRAY, over=JET, alpha=(7, 10)):
    """frames [N,224,298,ldf] float32, logen [N,36,48] float32 -> uint8 [N,224,298,3] through ops.overlay_render"""
    from acimg import ops
    N, ldf = frames.shape[0], frames.shape[3]
    plan = ops.Plan(device, eager=True)
    fr = torch.tensor(np.ascontiguousarray(frames, np.float32)).to(device)
    lg = torch.tensor(np.ascontiguousarray(logen, np.float32).reshape(N, 36 * 48)).to(device)
    bx = None if boxes is None else torch.tensor(np.ascontiguousarray(boxes, np.int32).reshape(N, 4, 3)).to(device)
    tb = torch.tensor(np.ascontiguousarray(base, np.uint8)).to(device)
    to = torch.tensor(np.ascontiguousarray(over, np.uint8)).to(device)
    out = torch.full((N, H, W, 3), 0x7B, dtype=torch.uint8, device=device)
    ops.overlay_render(plan, fr, ldf, lg, bx, tb, to, alpha[0], alpha[1], out, W * 3, H * W * 3, N)
    torch.cuda.synchronize(device)
    return out.cpu().numpy()


def ref_render(frames, logen, boxes=None, base=GRAY, over=JET, alpha=(7, 10)):
    return np.stack([ref.render(frames[n], logen[n], base, over, None if boxes is None else boxes[n], alpha)
                     for n in range(frames.shape[0])])


def assert_same_bytes(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at [n, y, x, c] = %s: got %d, want %d" % (
            what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def random_inputs(rng, N, ldf=3):
    frames = rng.rand(N, H, W, ldf).astype(np.float32)
    logen = (rng.rand(N, 36, 48) * rng.rand(N, 1, 1) * 3).astype(np.float32)      # scaled per sample
    return frames, logen


@pytest.fixture(scope="module")
def batch64():
    """one batch of 64 and its restatement, shared by the tests that need a reference (never modified)"""
    rng = np.random.RandomState(64)
    frames, logen = random_inputs(rng, 64)
    want = ref_render(frames, logen)
    for a in (frames, logen, want):
        a.setflags(write=False)
    return frames, logen, want


@pytest.mark.parametrize("N", [1, 7])
def test_overlay_equals_restatement(device, N):
    rng = np.random.RandomState(N)
    frames, logen = random_inputs(rng, N)
    assert_same_bytes(device_render(device, frames, logen), ref_render(frames, logen), "N = %d" % N)


def test_overlay_equals_restatement_64_and_replays(device, batch64):
    frames, logen, want = batch64
    got = device_render(device, frames, logen)
    assert_same_bytes(got, want, "N = 64")
    assert np.array_equal(device_render(device, frames, logen), got)               # replay: bit-identical


def test_overlay_with_boxes(device):
    rng = np.random.RandomState(17)
    frames, logen = random_inputs(rng, 9)
    boxes = random_boxes(rng, 9)
    boxes[0, :, 0] = (10, 20, 30, 40)
    boxes[1, :, 0] = (50, 52, 30, 40)                                              # narrower than 4: no interior
    boxes[2, :, 0] = (-2147483648, 2147483647, -2147483648, 2147483647)            # corners at the int32 limits
    boxes[3, :, 0] = (297, 1, 223, 1)                                              # reversed, on the frame's edge
    boxes[4, 1, :] = 0                                                             # all three absent
    got = device_render(device, frames, logen, boxes)
    assert_same_bytes(got, ref_render(frames, logen, boxes), "boxes")
    assert not np.array_equal(got[0], device_render(device, frames[:1], logen[:1])[0])   # the outline is there
    assert_same_bytes(got[4:5], ref_render(frames[4:5], logen[4:5]), "absent = no boxes")


def test_overlay_reads_three_of_ldf_channels(device, batch64):
    frames, logen, want = batch64
    f4 = np.full((5, H, W, 4), np.nan, np.float32)                                 # the fourth channel is poison
    f4[..., :3] = frames[:5]
    assert_same_bytes(device_render(device, f4, logen[:5]), want[:5], "ldf = 4")


def test_overlay_degenerate_samples_and_alpha_ends(device):
    rng = np.random.RandomState(5)
    frames, logen = random_inputs(rng, 4)
    frames[0], logen[0] = 0.4, 0.0                                                 # flat frame, flat map: entry 0 of both
    frames[1] = 0.7                                                                # flat frame under a live map
    logen[2] = 0.0415                                                              # constant map: last-place noise after
    logen[3, :, :24], logen[3, :, 24:] = 1.0, 2.0                                  # the resize, spread by the autoscale
    for alpha in ((7, 10), (0, 10), (10, 10), (1, 1), (0, 255), (254, 255)):
        got = device_render(device, frames, logen, alpha=alpha)
        assert_same_bytes(got, ref_render(frames, logen, alpha=alpha), "alpha %d / %d" % alpha)
    got = device_render(device, frames, logen)
    assert (got[0] == np.array([0, 0, 89], np.uint8)).all()
    base = np.stack([ref.colorize(ref.grey(f), GRAY) for f in frames])
    over = np.stack([ref.colorize(ref.resize_map(m), JET) for m in logen])
    assert_same_bytes(device_render(device, frames, logen, alpha=(0, 10)), base, "alpha 0 = base")
    assert_same_bytes(device_render(device, frames, logen, alpha=(10, 10)), over, "alpha 1 = overlay")


def test_overlay_uses_the_tables_it_is_given(device, batch64):
    frames, logen, _ = batch64
    rng = np.random.RandomState(8)
    tb, to = (rng.randint(0, 256, size=(256, 3)).astype(np.uint8) for _ in range(2))
    got = device_render(device, frames[:3], logen[:3], base=tb, over=to, alpha=(3, 7))
    assert_same_bytes(got, ref_render(frames[:3], logen[:3], base=tb, over=to, alpha=(3, 7)), "random tables")


def test_overlay_two_panels_inside_guard_bands(device, batch64):
    """the raw C ABI: two panels with a gap on one canvas whose rows have a tail (odd row_bytes: every 16-byte phase
    occurs), the workspace exactly the query's bytes and poisoned; gap, tails, image tails and guard bands stay"""
    from acimg import _lib, ops
    L = _lib.load()
    frames, logen, want = batch64
    N, gap, tail, SENT = 3, 5, 7, 0x7B
    rng = np.random.RandomState(2)
    logen_b = (rng.rand(N, 36, 48) * 0.01 + 0.04).astype(np.float32)
    want_b = ref_render(frames[:N], logen_b)
    row_bytes = (2 * W + gap) * 3 + tail
    image_bytes = H * row_bytes + 11
    q = int(L.acimg_overlay_render_workspace(N))
    arena = GuardArena.for_sizes(device, [N * image_bytes, q])
    canvas = arena.region(N * image_bytes, fill=SENT, name="canvas")
    ws = arena.region(q, fill=0xFF, name="ws")
    fr = torch.tensor(np.ascontiguousarray(frames[:N])).to(device)
    tb, to = torch.tensor(GRAY.copy()).to(device), torch.tensor(JET.copy()).to(device)
    st = ops.current_stream_handle(device)
    for lg_host, x0 in ((logen[:N], 0), (logen_b, W + gap)):
        lg = torch.tensor(np.ascontiguousarray(lg_host).reshape(N, 36 * 48)).to(device)
        rc = L.acimg_overlay_render(fr.data_ptr(), 3, lg.data_ptr(), None, tb.data_ptr(), to.data_ptr(), 7, 10,
                                    canvas.ptr + x0 * 3, row_bytes, image_bytes, N, ws.ptr, q, st)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize(device)
    arena.check("overlay_render")
    got = canvas.u8.cpu().numpy().reshape(N, image_bytes)
    assert (got[:, H * row_bytes:] == SENT).all()                                  # image tails
    rows = got[:, :H * row_bytes].reshape(N, H, row_bytes)
    assert (rows[:, :, (2 * W + gap) * 3:] == SENT).all()                          # row tails
    px = rows[:, :, :(2 * W + gap) * 3].reshape(N, H, 2 * W + gap, 3)
    assert (px[:, :, W:W + gap] == SENT).all()                                     # the gap keeps the canvas fill
    assert_same_bytes(px[:, :, :W], want[:N], "left panel")
    assert_same_bytes(px[:, :, W + gap:], want_b, "right panel")


def test_overlay_renderer_surface(device, batch64):
    from acimg.evaluate import OverlayRenderer
    from acimg.frontend import FrontEnd
    frames, logen, want = batch64
    rend = OverlayRenderer(device)
    f = torch.tensor(np.ascontiguousarray(frames[:4]))
    lg = torch.tensor(np.ascontiguousarray(logen[:4]))
    got = rend.render(f, lg)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, H, W, 3) and got.device.type == "cuda"
    assert_same_bytes(got.cpu().numpy(), want[:4], "render")
    out = torch.zeros(4, H, W, 3, dtype=torch.uint8, device=device)
    assert rend.render(f, lg.reshape(4, 1728), out=out) is out and torch.equal(out, got)
    # a 12-channel image goes through find_logen first
    rng = np.random.RandomState(4)
    img = torch.tensor(rng.rand(4, 36, 48, 12).astype(np.float32)).to(device)
    en = FrontEnd(device).find_logen(img).cpu().numpy()
    assert_same_bytes(rend.render(f, img).cpu().numpy(), ref_render(frames[:4], en), "12 channels")
    pair = rend.render_pair(f, lg, img, gap=6).cpu().numpy()
    assert pair.shape == (4, H, 2 * W + 6, 3) and (pair[:, :, W:W + 6] == 255).all()
    assert_same_bytes(pair[:, :, :W], want[:4], "pair, left = real")
    assert_same_bytes(pair[:, :, W + 6:], ref_render(frames[:4], en), "pair, right = generated")
    other = OverlayRenderer(device, base=JET, over="gray", alpha=(1, 4))
    assert_same_bytes(other.render(f, lg).cpu().numpy(), ref_render(frames[:4], logen[:4], base=JET, over=GRAY, alpha=(1, 4)),
                      "other")
    with pytest.raises(ValueError):
        OverlayRenderer(device, alpha=(11, 10))
    with pytest.raises(ValueError):
        rend.render(f[:, :100], lg)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_show_end_to_end(device, tmp_path):
    from acimg import show, tfio
    from acimg.data import BoxRecordLoader, TFRecordDataLoader
    from acimg.flags import FLAGS
    from acimg.frontend import FrontEnd
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    rng = np.random.RandomState(31)
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    src = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                  ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    src._build_functions(batch_size=3)
    src.modelimages.initialize()
    src.modelac.initialize()
    state = OrderedDict((k, v.numpy()) for k, v in src.session.store.state_dict().items())
    ckdir = tmp_path / "ckpt"
    ckdir.mkdir()
    ckpt = str(ckdir / "epoch_7.ckpt")
    tfio.write_checkpoint(ckpt, state)

    vdir = tmp_path / "class_1" / "video_4"
    vdir.mkdir(parents=True)
    ofiles = [str(vdir / "o0.tfrecord"), str(vdir / "o1.tfrecord")]
    tfio.write_tfrecord(ofiles[0], [outdoor_record(rng, 2, 7, wide=False)], compression="GZIP")
    tfio.write_tfrecord(ofiles[1], [outdoor_record(rng, 4, 7, wide=False)], compression="GZIP")
    olist = vdir / "testing.txt"
    olist.write_text("\n".join(ofiles) + "\n")
    common = ["--init_checkpoint", ckpt, "--batch_size", "3", "--num_skip_conn", "1", "--ae", "0", "--png_level", "1"]

    def load_png(path):
        with open(path, "rb") as f:
            return read_png(f.read())

    vargs = show.parse_args(["video", "--train_file", str(olist)] + common)
    tr = show.build_trainer(vargs, device)
    res = show.run(vargs, trainer=tr, keep_energy=True, log=lambda *a: None)
    batches = list(TFRecordDataLoader(str(olist), 3, device=device).data)
    frames = np.concatenate([b[2].numpy() for b in batches])
    energy = res["energy"].reshape(-1, 36, 48)
    assert res["num_frames"] == 24 and energy.shape[0] == 24 and np.isfinite(energy).all() and np.ptp(energy[0]) > 0
    d = show.output_dir(vargs)
    assert d == str(vdir / "Generated_10s") and sorted(os.listdir(d)) == sorted(
        ["I_%06d.png" % i for i in range(24)] + ["show.json"])
    for i in range(24):
        assert_same_bytes(load_png(os.path.join(d, "I_%06d.png" % i)), ref.render(frames[i], energy[i], GRAY, JET),
                          "video frame %d" % i)
    with open(os.path.join(d, "show.json")) as f:
        js = json.load(f)
    assert js["num_frames"] == 24 and js["fps"] == 12 and js["printf_pattern"] == "I_%06d.png" and len(js["ffmpeg"]) == 2
    assert js["ffmpeg"][1].endswith("/video_boat_video_4_7.avi")

    iargs = show.parse_args(["images", "--train_file", str(olist)] + common)
    res = show.run(iargs, trainer=tr, keep_energy=True, log=lambda *a: None)
    energy = res["energy"].reshape(-1, 36, 48)
    fe = FrontEnd(device)
    real = np.concatenate([fe.find_logen(b[0].to(device)).cpu().numpy() for b in batches])
    assert np.array_equal(res["energy_real"].reshape(-1, 36, 48), real)
    d = show.output_dir(iargs)
    assert d == str(ckdir / "UNet_testing_AcousticMapJet_7") and res["width"] == 2 * W + show.GAP
    for i in range(24):
        img = load_png(os.path.join(d, "testing_images_%d.png" % i))
        assert img.shape == (H, 2 * W + show.GAP, 3) and (img[:, W:W + show.GAP] == 255).all()
        assert_same_bytes(img[:, :W], ref.render(frames[i], real[i], GRAY, JET), "real %d" % i)
        assert_same_bytes(img[:, W + show.GAP:], ref.render(frames[i], energy[i], GRAY, JET), "generated %d" % i)

    bfiles = [str(tmp_path / "f0.tfrecord")]
    tfio.write_tfrecord(bfiles[0], [random_box_record(rng, 12288), random_box_record(rng, 24576), random_box_record(rng, 15001)],
                        compression="GZIP")
    blist = tmp_path / "flickr_test.txt"
    blist.write_text("\n".join(bfiles) + "\n")
    bargs = show.parse_args(["boxes", "--train_file", str(blist)] + common)
    res = show.run(bargs, trainer=tr, keep_energy=True, log=lambda *a: None)
    energy = res["energy"].reshape(-1, 36, 48)
    bb = list(BoxRecordLoader(str(blist), 3).data)
    frames = np.concatenate([b[2].numpy() for b in bb])
    boxes = np.concatenate([torch.stack(list(b[3:7]), 1).numpy() for b in bb])
    d = show.output_dir(bargs)
    assert d == str(ckdir / "UNet_flickr_test_AcousticFramesJet2_7") and res["num_frames"] == 3
    for i in range(3):
        assert_same_bytes(load_png(os.path.join(d, "flickr_test_images_%d.png" % i)),
                          ref.render(frames[i], energy[i], GRAY, JET, boxes=boxes[i]), "boxes %d" % i)
