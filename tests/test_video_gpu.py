"""The demo clip on the device: `acimg_jpeg_blocks` and `acimg_jpeg_scan` against the NumPy restatement (tests/jpeg_ref.py)
byte for byte inside guard bands, `JpegEncoder.encode` as complete files (and, where PIL imports, decoded by libjpeg
within 0.1 dB of libjpeg's own file at the same tables), and `python -m acimg.show video --avi 1` end to end: the PNG
frames and show.json as before, the AVI's pictures equal to the restatement's encoding of the PNG pixels, its sound
equal to the records' samples normalised to the clip's peak."""
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

import avi_support  # noqa: E402
import jpeg_ref as J  # noqa: E402
from data_support import outdoor_arrays, outdoor_example  # noqa: E402
from guard_arena import GuardArena  # noqa: E402
import render_ref  # noqa: E402
from render_ref import read_png  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "render_golden.npz"))
SENT = 0x7B


@pytest.fixture(scope="module")
def overlay():
    img = J.overlay_image(GOLD["table_gray"], GOLD["table_jet"])
    img.setflags(write=False)
    return img


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: got %d, want %d" % (
            what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W", [(1, 16, 16), (2, 17, 33), (1, 224, 298)])
def test_blocks_equal_restatement(device, overlay, n, H, W):
    from acimg import _lib, ops
    L = _lib.load()
    inputs = (("noise", np.stack([J.noise_image(H, W, 10 * H + i) for i in range(n)])),
              ("flat 200", np.full((n, H, W, 3), 200, np.uint8)),
              ("overlay", np.stack([np.ascontiguousarray(overlay[i:i + H, 2 * i:2 * i + W]) for i in range(n)])))
    nbytes = int(L.acimg_jpeg_coef_bytes(n, H, W))
    mcus = -(-H // 16) * -(-W // 16)
    assert nbytes == n * mcus * 768
    st = ops.current_stream_handle(device)
    for name, frames in inputs:
        rgb = torch.from_numpy(frames).to(device)
        for quality in (50, 90, 100):
            qt = J.quant_tables(quality)
            arena = GuardArena.for_sizes(device, [nbytes])
            out = arena.region(nbytes, fill=SENT, name="coef")
            qd = torch.from_numpy(qt.reshape(128).copy()).to(device)
            rc = L.acimg_jpeg_blocks(rgb.data_ptr(), n, H, W, qd.data_ptr(), out.ptr, st)
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize(device)
            arena.check("jpeg_blocks %s q %d" % (name, quality))
            got = out.view(torch.int16, n, mcus, 6, 64).cpu().numpy()
            want = np.stack([J.blocks(f, qt) for f in frames])                  # padded MCUs included
            same_bytes(got, want, "%s %dx%dx%d q %d" % (name, n, H, W, quality))
            if name == "flat 200":
                assert (got[..., 1:] == 0).all() and (got[:, :, :4, 0] != 0).all()


# ---- scan -------------------------------------------------------------------------------------------------------------
def device_scan(device, coef, H, W, restart, slack=5):
    """-> (scan bytes per frame, the whole output region as a host array, stride); guard bands checked"""
    from acimg import _lib, ops
    L = _lib.load()
    n = coef.shape[0]
    cap = int(L.acimg_jpeg_scan_capacity(H, W, restart))
    assert cap == J.scan_capacity(H, W, restart)
    stride = cap + slack
    wsb = int(L.acimg_jpeg_scan_workspace(n, H, W, restart))
    arena = GuardArena.for_sizes(device, [n * stride, 4 * n, wsb])
    out = arena.region(n * stride, fill=SENT, name="scan")
    cnt = arena.region(4 * n, fill=0xFF, name="scan_bytes")
    ws = arena.region(wsb, fill=0xEE, name="ws")
    cd = torch.from_numpy(np.ascontiguousarray(coef)).to(device)
    rc = L.acimg_jpeg_scan(cd.data_ptr(), n, H, W, restart, out.ptr, stride, cnt.ptr, ws.ptr, wsb,
                           ops.current_stream_handle(device))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check("jpeg_scan %dx%d r %d" % (H, W, restart))
    return cnt.view(torch.int32, n).cpu().numpy(), out.u8.cpu().numpy().reshape(n, stride), cap


@pytest.mark.parametrize("n,H,W", [(2, 17, 33), (1, 32, 144), (1, 48, 368), (1, 224, 298)])
@pytest.mark.parametrize("full", [False, True])
def test_scan_equals_restatement(device, n, H, W, full):
    """(1, 48, 368): 69 MCUs, so the merge kernel's 64-MCU scan takes a second pass - restart 69 is 64 + 5 MCUs, restart
    65 is 64 + 1 and then an interval of 4.  (1, 224, 298): 266 MCUs - restart 1 is 266 intervals, two for some pack
    threads and one for others, the RSTm index wrapping 33 times; restart 266 is one interval of five scan passes"""
    mh, mw = J.mcu_grid(H, W)
    mcus = mh * mw
    coef = J.synthetic_coefficients(n, mcus, full)
    for restart in (1, mw, 7, mcus) + ((65,) if mcus == 69 else ()):
        counts, region, cap = device_scan(device, coef, H, W, restart)
        for i in range(n):
            want = J.scan(coef[i], restart)
            assert counts[i] == len(want) <= cap, (restart, i, counts[i], len(want), cap)
            same_bytes(region[i, :counts[i]], np.frombuffer(want, np.uint8), "r %d frame %d" % (restart, i))
            assert (region[i, counts[i]:] == SENT).all()                         # the rest of the slot is untouched
            markers = J.num_intervals(H, W, restart) - 1
            assert [want.count(bytes([0xFF, 0xD0 + m])) for m in range(8)] == [
                len(range(m, markers, 8)) for m in range(8)]
            if full:
                assert b"\xFF\x00" in want                                        # stuffing occurred
        again, region2, _ = device_scan(device, coef, H, W, restart)
        assert np.array_equal(again, counts) and np.array_equal(region2, region)  # bit-identical from run to run
    if (H, W) == (32, 144):
        assert J.num_intervals(H, W, 1) == 18 and J.num_intervals(H, W, 7) == 3   # the index wraps; a short last interval
    if (H, W) == (48, 368):
        assert mcus == 69 and J.num_intervals(H, W, 65) == 2
    if (H, W) == (224, 298):
        assert mcus == 266 and J.num_intervals(H, W, 1) == 266 and J.num_intervals(H, W, 266) == 1


# ---- the encoder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W", [(2, 17, 33), (1, 224, 298)])
def test_encoder_files_equal_restatement(device, overlay, n, H, W):
    from acimg.jpeg import JpegEncoder
    if (H, W) == (224, 298):
        frames = np.array(overlay[None])
    else:
        frames = np.stack([J.noise_image(H, W, 40 + i) for i in range(n)])
        frames[1, :, 16:] = frames[1, :, 16:] // 16 + 90
    for quality, restart in ((90, None), (50, 7)):
        enc = JpegEncoder(device, quality=quality, restart_mcus=restart)
        files = enc.encode(torch.from_numpy(np.ascontiguousarray(frames)).to(device))
        assert len(files) == n and all(isinstance(f, bytes) for f in files)
        for i in range(n):
            assert files[i] == J.encode(frames[i], quality, restart), (quality, restart, i)
        assert enc.encode(torch.from_numpy(np.ascontiguousarray(frames))) == files           # a host tensor is copied up
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    files = JpegEncoder(device, quality=90).encode(torch.from_numpy(np.ascontiguousarray(frames)).to(device))
    for i in range(n):
        ours, theirs = J.psnr_pair(frames[i], files[i], 90)
        print("device file %dx%d frame %d: ours %.3f dB, libjpeg %.3f dB" % (H, W, i, ours, theirs))
        assert ours >= theirs - J.MARGIN_DB


def test_write_jpeg(device, tmp_path):
    from acimg.jpeg import write_jpeg
    img = J.noise_image(17, 33, 9)
    path = str(tmp_path / "a.jpg")
    size = write_jpeg(path, img, quality=75, device=device)
    with open(path, "rb") as f:
        data = f.read()
    assert size == len(data) and data == J.encode(img, 75, None)
    with pytest.raises(ValueError):
        write_jpeg(path, img[..., :2], device=device)


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_show_video_avi_end_to_end(device, tmp_path):
    from acimg import show, tfio
    from acimg.avi import normalize_pcm
    from acimg.data import TFRecordDataLoader
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    rng = np.random.RandomState(31)
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    src = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                  ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    src._build_functions(batch_size=5)
    src.modelimages.initialize()
    src.modelac.initialize()
    state = OrderedDict((k, v.numpy()) for k, v in src.session.store.state_dict().items())
    ckdir = tmp_path / "ckpt"
    ckdir.mkdir()
    ckpt = str(ckdir / "epoch_7.ckpt")
    tfio.write_checkpoint(ckpt, state)

    ai, sa, vi = outdoor_arrays(rng, wide=False)
    sa[3, 17] = -30000                                                           # the clip's peak is a negative sample
    record = outdoor_example(ai, sa, vi, 2, 7)
    lists = []
    for name in ("with", "without"):                                            # one record of 12 frames in each
        vdir = tmp_path / name / "class_1" / "video_4"
        vdir.mkdir(parents=True)
        tfio.write_tfrecord(str(vdir / "o0.tfrecord"), [record], compression="GZIP")
        (vdir / "testing.txt").write_text(str(vdir / "o0.tfrecord") + "\n")
        lists.append(str(vdir / "testing.txt"))
    common = ["--init_checkpoint", ckpt, "--batch_size", "5", "--num_skip_conn", "1", "--ae", "0", "--png_level", "1"]

    args = show.parse_args(["video", "--train_file", lists[0], "--avi", "1", "--quality", "90"] + common)
    tr = show.build_trainer(args, device)
    res = show.run(args, trainer=tr, keep_energy=True, log=lambda *a: None)
    d = show.output_dir(args)
    vdir = os.path.dirname(lists[0])
    assert d == os.path.join(vdir, "Generated_10s")
    assert sorted(os.listdir(d)) == sorted(["I_%06d.png" % i for i in range(12)] + ["show.json"])
    avi_path = os.path.join(vdir, "video_boat_video_4_7.avi")
    assert sorted(os.listdir(vdir)) == sorted(["Generated_10s", "o0.tfrecord", "testing.txt", "video_boat_video_4_7.avi"])
    with open(os.path.join(d, "show.json")) as f:
        js = json.load(f)
    assert js == {k: res[k] for k in js}
    assert js["num_frames"] == 12 and js["fps"] == 12 and js["printf_pattern"] == "I_%06d.png" and len(js["ffmpeg"]) == 2
    assert js["command"] == "video" and js["file_pattern"] == "I_{:06d}.png" and js["directory"] == d
    assert (js["height"], js["width"], js["checkpoint"]) == (224, 298, ckpt)
    assert js["ffmpeg"][1].endswith(" " + avi_path)
    assert js["avi"] == avi_path and js["avi_bytes"] == os.path.getsize(avi_path)
    assert (js["quality"], js["restart_mcus"], js["sample_rate"]) == (90, 19, 12288)

    with open(avi_path, "rb") as f:
        avi = avi_support.parse(f.read())
    ch = avi["chunks"]
    assert [c["fourcc"] for c in ch] == [b"00dc", b"01wb"] * 12
    assert avi["avih"]["dwTotalFrames"] == 12 and avi["streams"][0]["strh"]["dwLength"] == 12
    assert avi["streams"][0]["strh"]["dwRate"] == 12 and avi["streams"][1]["strh"]["dwRate"] == 12288
    assert avi["streams"][1]["strh"]["dwLength"] == 12 * 1024 and len(avi["index"]) == 24
    batches = list(TFRecordDataLoader(lists[0], 5, device=device, raw_audio=True).data)
    frames = np.concatenate([b[2].numpy() for b in batches])
    energy = res["energy"].reshape(12, 36, 48)
    for i in range(12):
        with open(os.path.join(d, "I_%06d.png" % i), "rb") as f:
            png = read_png(f.read())
        same_bytes(png, render_ref.render(frames[i], energy[i], GOLD["table_gray"], GOLD["table_jet"]), "frame %d" % i)
        assert ch[2 * i]["data"] == J.encode(png, 90, None), "picture %d" % i
    pcm = np.frombuffer(b"".join(ch[2 * i + 1]["data"] for i in range(12)), "<i2")
    want = np.rint(sa.reshape(-1).astype(np.float64) / 30000.0 * 32767.0).astype(np.int16)
    assert np.array_equal(pcm, want) and pcm.min() == -32767 and np.array_equal(pcm, normalize_pcm(sa))
    # the seventh tensor is the records' audio, re-batched like the rest (5 + 5 + 2)
    assert [len(b) for b in batches] == [7, 7, 7] and [b[6].shape[0] for b in batches] == [5, 5, 2]
    assert batches[0][6].dtype == torch.int32 and np.array_equal(np.concatenate([b[6].numpy() for b in batches]), sa)
    assert all(len(b) == 6 for b in TFRecordDataLoader(lists[0], 5, device=device).data)

    # without the flag: frames and summary as ever, and no AVI (the generator samples, so the pictures differ run to run)
    args0 = show.parse_args(["video", "--train_file", lists[1], "--avi", "0"] + common)
    res0 = show.run(args0, trainer=tr, log=lambda *a: None)
    d0, vdir0 = show.output_dir(args0), os.path.dirname(lists[1])
    assert sorted(os.listdir(vdir0)) == sorted(["Generated_10s", "o0.tfrecord", "testing.txt"])
    assert sorted(os.listdir(d0)) == sorted(["I_%06d.png" % i for i in range(12)] + ["show.json"])
    assert list(res0) == ["command", "num_frames", "file_pattern", "directory", "height", "width", "checkpoint", "fps",
                          "printf_pattern", "ffmpeg"]
    assert list(js)[:len(res0)] == list(res0)
    for k in ("command", "num_frames", "file_pattern", "height", "width", "checkpoint", "fps", "printf_pattern"):
        assert res0[k] == js[k]
    with open(os.path.join(d0, "show.json")) as f:
        assert json.load(f) == res0
    with open(os.path.join(d0, "I_000011.png"), "rb") as f:
        assert read_png(f.read()).shape == (224, 298, 3)
