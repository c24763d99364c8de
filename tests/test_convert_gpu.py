"""The dataset converter on the device: `acimg_resize_cubic_u8` against the NumPy restatement of OpenCV's fixed-point
INTER_CUBIC (tests/convert_ref.py) bit for bit, inside guard bands, on BMP-shaped operands (odd pixel offset, padded and
bottom-up rows), on every path of the kernel (one tile, several column tiles, a band worked off in chunks, several
frames), twice each; its refusals; and `python -m acimg.convert` end to end on a raw tree written here, read back through
`tfio`, `TFRecordDataLoader(..., modalities=(1, 2))` and `python -m acimg.show video`."""
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

import convert_ref as ref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B


def assert_equal_frames(got, want, what=""):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at [n, y, x, c] = %s: got %d, want %d" % (
            what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


class Operand(object):
    """n frames as the C ABI sees them: `lead` bytes, then per frame `frame_stride` bytes with the top row at
    `pixel_offset` and rows `row_stride` apart"""

    def __init__(self, frames, pitch=None, bottom_up=False, header=0, tail=0, lead=0, rng=None):
        n, H, W = frames.shape[:3]
        pitch = 3 * W if pitch is None else pitch
        rng = rng or np.random.RandomState(0)
        self.frame_stride = header + H * pitch + tail
        buf = rng.randint(0, 256, size=lead + n * self.frame_stride).astype(np.uint8)      # padding and gaps are noise
        for i in range(n):
            rows = buf[lead + i * self.frame_stride + header:][:H * pitch].reshape(H, pitch)
            rows[::-1 if bottom_up else 1, :3 * W] = frames[i].reshape(H, 3 * W)
        self.bytes, self.lead, self.n, self.H, self.W = buf, lead, n, H, W
        self.pixel_offset = header + ((H - 1) * pitch if bottom_up else 0)
        self.row_stride = -pitch if bottom_up else pitch


def device_resize(device, op, new_size, window=None, runs=2, what=""):
    """the raw C ABI, source and output inside guard bands; every run must give the same bytes"""
    from acimg import _lib, ops
    L = _lib.load()
    y0, x0, OH, OW = window if window is not None else (0, 0) + tuple(new_size)
    tabs = ref.cubic_tables(op.H, new_size[0], y0, OH) + ref.cubic_tables(op.W, new_size[1], x0, OW)
    dev_tabs = [torch.from_numpy(t).to(device) for t in tabs]
    out_bytes = op.n * OH * OW * 3
    arena = GuardArena.for_sizes(device, [op.bytes.size, out_bytes])
    src = arena.region(op.bytes.size, name="src")
    src.u8.copy_(torch.from_numpy(op.bytes))
    out = arena.region(out_bytes, name="out")
    got = []
    for _ in range(runs):
        out.fill(SENT)
        rc = L.acimg_resize_cubic_u8(src.ptr + op.lead, op.frame_stride, op.pixel_offset, op.row_stride, op.n, op.H, op.W,
                                     *[t.data_ptr() for t in dev_tabs], OH, OW, out.ptr, ops.current_stream_handle(device))
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize(device)
        arena.check(what)
        got.append(out.u8.cpu().numpy().reshape(op.n, OH, OW, 3))
    assert torch.equal(src.u8.cpu(), torch.from_numpy(op.bytes)), "the source was written"
    for g in got[1:]:
        assert np.array_equal(g, got[0]), "%s: two runs differ" % what
    return got[0]


def ref_resize(frames, new_size, window=None):
    return np.stack([ref.resize_cubic(f, new_size[0], new_size[1], window) for f in frames])


def test_one_bmp_frame_480x640(device):
    """a 640 x 480 bottom-up BMP as it lies in the file: pixels from byte 54, one launch -> 224 x 298"""
    rng = np.random.RandomState(1)
    frames = rng.randint(0, 256, size=(1, 480, 640, 3)).astype(np.uint8)
    op = Operand(frames, bottom_up=True, header=54, rng=rng)
    got = device_resize(device, op, (224, 298), what="480x640")
    assert_equal_frames(got, ref_resize(frames, (224, 298)), "480x640 -> 224x298")
    assert_equal_frames(got[0], ref.convert_frame(frames[0]), "convert_frame")


def test_three_padded_top_down_frames_upscaled_with_crop(device):
    """53 x 37 (W x H), rows padded to 160 bytes, top-down, an odd base address: -> 224 x 320, window 224 x 298 at x = 11"""
    rng = np.random.RandomState(2)
    frames = rng.randint(0, 256, size=(3, 37, 53, 3)).astype(np.uint8)
    op = Operand(frames, pitch=160, header=54, tail=3, lead=1, rng=rng)
    assert ref.smallest_size_at_least(37, 53) == (224, 320)
    win = (0, 11, 224, 298)
    assert_equal_frames(device_resize(device, op, (224, 320), win, what="53x37"), ref_resize(frames, (224, 320), win), "53x37")


def test_small_window_with_crop_offsets(device):
    """11 x 23 (W x H) -> 9 x 12 (h x w), of which the 5 x 7 (w x h) window at (y, x) = (1, 4)"""
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=(1, 23, 11, 3)).astype(np.uint8)
    op = Operand(frames, pitch=36, bottom_up=True, header=54, rng=rng)
    win = (1, 4, 7, 5)
    assert_equal_frames(device_resize(device, op, (9, 12), win, what="11x23"), ref_resize(frames, (9, 12), win), "11x23")


def test_checkerboard_saturates_at_both_ends(device):
    """0 / 255 squares of one and of three pixels: the negative lobes overshoot below 0 and above 255, the clamp holds"""
    y, x = np.mgrid[0:48, 0:64]
    one = (((y + x) & 1) * 255).astype(np.uint8)
    three = ((((y // 3) + (x // 3)) & 1) * 255).astype(np.uint8)
    frames = np.stack([np.repeat(one[..., None], 3, 2), np.repeat(three[..., None], 3, 2)])
    op = Operand(frames, bottom_up=True, header=54)
    for size in ((224, 298), (37, 50)):
        want = ref_resize(frames, size)
        assert want.min() == 0 and want.max() == 255
        assert_equal_frames(device_resize(device, op, size, what="checkerboard"), want, "checkerboard -> %d x %d" % size)


def test_thirteen_frames(device):
    rng = np.random.RandomState(4)
    frames = rng.randint(0, 256, size=(13, 48, 64, 3)).astype(np.uint8)
    op = Operand(frames, bottom_up=True, header=54, tail=2, rng=rng)
    assert_equal_frames(device_resize(device, op, (30, 40), what="13 frames"), ref_resize(frames, (30, 40)), "13 frames")


def test_every_kernel_path(device):
    """several column tiles (more than 320 output columns); a band whose source rows exceed the LDS tile and is worked
    off in chunks (480 -> 16 and -> 40 rows at 298 columns: 30 and 12 source rows per output row, 20 in the tile, so one
    and two output rows per chunk); output rows that are no multiple of the band"""
    rng = np.random.RandomState(5)
    small = rng.randint(0, 256, size=(2, 13, 29, 3)).astype(np.uint8)
    op = Operand(small, pitch=88, header=54, rng=rng)
    assert_equal_frames(device_resize(device, op, (61, 701), what="wide"), ref_resize(small, (61, 701)), "13x29 -> 61x701")
    big = rng.randint(0, 256, size=(1, 480, 640, 3)).astype(np.uint8)
    op = Operand(big, bottom_up=True, header=54, rng=rng)
    assert_equal_frames(device_resize(device, op, (16, 298), what="steep"), ref_resize(big, (16, 298)), "480x640 -> 16x298")
    assert_equal_frames(device_resize(device, op, (40, 298), runs=1, what="two rows a chunk"), ref_resize(big, (40, 298)),
                      "480x640 -> 40x298")


def test_refusals_leave_output_and_guard_bands_untouched(device):
    from acimg import _lib, ops
    L = _lib.load()
    H, W, OH, OW, n = 10, 12, 5, 6, 2
    pitch, off = 36, 54
    fs = off + H * pitch
    tabs = [torch.from_numpy(t).to(device) for t in ref.cubic_tables(H, OH) + ref.cubic_tables(W, OW)]
    iy, cy, ix, cx = [t.data_ptr() for t in tabs]
    arena = GuardArena.for_sizes(device, [n * fs, n * OH * OW * 3])
    src = arena.region(n * fs, fill=1, name="src")
    out = arena.region(n * OH * OW * 3, fill=SENT, name="out")
    st = ops.current_stream_handle(device)
    top = off + (H - 1) * pitch
    good = [src.ptr, fs, off, pitch, n, H, W, iy, cy, ix, cx, OH, OW, out.ptr, st]
    bad = []
    for i in (0, 7, 8, 9, 10, 13):                                   # a null pointer
        bad.append(good[:i] + [None] + good[i + 1:])
    for i in (4, 5, 6, 11, 12):                                      # a non-positive size
        bad.append(good[:i] + [0] + good[i + 1:])
        bad.append(good[:i] + [-3] + good[i + 1:])
    bad.append(good[:3] + [3 * W - 1] + good[4:])                    # |row_stride| < 3 W
    bad.append(good[:3] + [-(3 * W - 1)] + good[4:])
    bad.append(good[:1] + [fs - pitch + 3 * W - 1] + good[2:])       # top-down: the last row overruns frame_stride
    bad.append(good[:2] + [off + pitch + 1] + good[3:])
    bad.append(good[:2] + [(H - 1) * pitch - 1, -pitch] + good[4:])  # bottom-up: the last row lies before the frame
    bad.append(good[:1] + [top + 3 * W - 1, top, -pitch] + good[4:])     # bottom-up: the top row overruns frame_stride
    for args in bad:
        assert L.acimg_resize_cubic_u8(*args) == -1, args
        assert "resize_cubic_u8" in _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check("refusals")
    assert bool((out.u8 == SENT).all()) and bool((src.u8 == 1).all())
    # the tightest operands that are taken: exactly-fitting strides, both directions
    for args in (good[:1] + [fs - pitch + 3 * W] + good[2:], good[:1] + [top + 3 * W, top, -pitch] + good[4:]):
        assert L.acimg_resize_cubic_u8(*args) == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check("tight operands")


def test_frame_resizer(device):
    from acimg.convert import FrameResizer
    rng = np.random.RandomState(6)
    frames = rng.randint(0, 256, size=(2, 480, 640, 3)).astype(np.uint8)
    rs = FrameResizer(device, 480, 640)
    assert rs.new_size == (224, 298) and rs.window == (0, 0, 224, 298)
    got = rs.resize_frames(frames)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 224, 298, 3) and got.device.type == "cuda"
    assert_equal_frames(got.cpu().numpy(), np.stack([ref.convert_frame(f) for f in frames]), "FrameResizer")
    other = FrameResizer(device, 480, 640, new_size=(100, 90), window=(3, 5, 40, 30))
    assert_equal_frames(other.resize_frames(frames).cpu().numpy(), ref_resize(frames, (100, 90), (3, 5, 40, 30)), "window")
    with pytest.raises(ValueError):
        rs.resize_frames(frames[:, :100])


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def converted(device, tmp_path_factory):
    """a raw tree of two recordings (2 s; video_time 0) of 640 x 480 frames, converted once; the restatement of its frames
    (never modified)"""
    from acimg import convert
    rng = np.random.RandomState(11)
    root = tmp_path_factory.mktemp("convert")
    raw, out = root / "raw", root / "out"
    raw.mkdir()
    out.mkdir()
    frames = rng.randint(0, 256, size=(24, 480, 640, 3)).astype(np.uint8)
    sound = rng.randint(-2 ** 15, 2 ** 15, size=2 * 12288 + 33)
    ref.write_recording(raw, 3, 7, 2, frames, sound)
    ref.write_recording(raw, 3, 8, 0, frames[:1], sound)
    lst = str(out / "testing.txt")
    assert convert.main([str(raw), str(out), "--list", lst, "--device", str(device), "--workers", "3"]) == 0
    want = np.stack([ref.convert_frame(f) for f in frames])
    audio = sound[:2 * 12288].astype(np.int32).reshape(24, 1024)
    for a in (want, audio):
        a.setflags(write=False)
    return dict(out=str(out), list=lst, video=want, audio=audio)


def test_convert_end_to_end(converted):
    from acimg import tfio
    out = converted["out"]
    paths = [os.path.join(out, "class_3", "data_007", "Data_%03d.tfrecord" % k) for k in (1, 2)]
    # (Generated_10s is the show test's, written beside the list)
    assert set(os.listdir(out)) - {"Generated_10s"} == {"class_3", "testing.txt"}
    assert os.listdir(os.path.join(out, "class_3")) == ["data_007"]
    assert sorted(os.listdir(os.path.dirname(paths[0]))) == ["Data_001.tfrecord", "Data_002.tfrecord"]
    assert open(converted["list"]).read() == "".join(p + "\n" for p in paths)
    for k, p in enumerate(paths):
        with open(p, "rb") as f:
            assert f.read(2) == b"\x1f\x8b"                                   # GZIP
        (rec,) = list(tfio.read_tfrecord(p))
        ctx, lists = tfio.parse_sequence_example(rec)
        assert list(ctx) == ["classes", "location", "audio_data/mics", "audio_data/samples", "video/height", "video/width",
                             "video/depth"]
        assert [int(v[0]) for v in ctx.values()] == [3, 7, 1, 1024, 224, 298, 3]
        assert list(lists) == ["audio/data", "video/image"] and all(len(v) == 12 for v in lists.values())
        video = np.stack([np.frombuffer(s[0], np.uint8).reshape(224, 298, 3) for s in lists["video/image"]])
        assert_equal_frames(video, converted["video"][12 * k:12 * k + 12], "record %d" % (k + 1))
        audio = np.stack([np.frombuffer(s[0], "<i4") for s in lists["audio/data"]])
        assert np.array_equal(audio, converted["audio"][12 * k:12 * k + 12])


def test_loader_reads_converted_records(device, converted):
    from acimg.data import TFRecordDataLoader
    from acimg.frontend import FrontEnd
    batches = list(TFRecordDataLoader(converted["list"], 4, device=device, modalities=(1, 2)).data)
    assert len(batches) == 6 and all(len(b) == 6 for b in batches)
    for b in batches:
        assert b[0].dtype == torch.float32 and tuple(b[0].shape) == (4, 36, 48, 12) and not b[0].any()
    video = torch.cat([b[2] for b in batches]).numpy()
    assert np.array_equal(video, converted["video"][..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0))
    fe = FrontEnd(device)
    mfcc = torch.cat([fe._build_spectrograms_function(torch.from_numpy(converted["audio"][k:k + 12].copy()).to(device),
                                                      normalize=True).cpu() for k in (0, 12)])
    assert torch.equal(torch.cat([b[1] for b in batches]), mfcc)
    act, loc = torch.cat([b[3] for b in batches]), torch.cat([b[4] for b in batches])
    assert tuple(act.shape) == (24, 10) and bool((act.argmax(1) == 3).all()) and bool((act.sum(1) == 1).all())
    assert tuple(loc.shape) == (24, 61) and bool((loc.argmax(1) == 7).all())
    with pytest.raises(ValueError, match="acoustic"):
        list(TFRecordDataLoader(converted["list"], 4, device=device).data)


def test_show_video_plays_converted_records(device, converted, tmp_path):
    from acimg import show, tfio
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    src = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                  ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    src._build_functions(batch_size=3)
    src.modelimages.initialize()
    src.modelac.initialize()
    state = OrderedDict((k, v.numpy()) for k, v in src.session.store.state_dict().items())
    ckpt = str(tmp_path / "epoch_7.ckpt")
    tfio.write_checkpoint(ckpt, state)
    argv = ["video", "--train_file", converted["list"], "--init_checkpoint", ckpt, "--batch_size", "3", "--num_skip_conn",
            "1", "--ae", "0", "--png_level", "1", "--device", str(device)]
    assert show.main(argv) == 0
    d = os.path.join(converted["out"], "Generated_10s")
    assert sorted(os.listdir(d)) == sorted(["I_%06d.png" % i for i in range(24)] + ["show.json"])
    with open(os.path.join(d, "show.json")) as f:
        js = json.load(f)
    assert js["num_frames"] == 24 and js["fps"] == 12 and js["printf_pattern"] == "I_%06d.png"
