"""Visualisation without a GPU: the colour tables and the index rule against matplotlib's own output
(tests/golden/render_golden.npz, written by tests/golden/make_render_golden.py), hand-computed cases of the overlay rule
as `render_ref` restates it, the PNG writer read back by a reader written here, `python -m acimg.show`'s arguments,
directories, file names and `show.json`, and the refusals of `acimg_overlay_render`, which come before any launch."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import render_ref as ref  # noqa: E402
from localize_ref import boxes_of  # noqa: E402
from render_ref import read_png  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "render_golden.npz"))
GOLD_INPUTS = sorted(k[3:] for k in GOLD.files if k.startswith("in_"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


# ---- colour stage: pinned against matplotlib -------------------------------------------------------------------------
def test_colormap_tables_equal_matplotlib():
    from acimg import colormaps
    for name in ("jet", "gray"):
        t = colormaps.byte_table(name)
        assert t.dtype == np.uint8 and t.shape == (256, 3)
        assert np.array_equal(t, GOLD["table_" + name]), name
    # the grey table is not the identity: truncation of i / 255 * 255 leaves 24 entries at i - 1
    assert int((GOLD["table_gray"][:, 0] != np.arange(256)).sum()) == 24
    with pytest.raises(ValueError):
        colormaps.byte_table("viridis")


def test_golden_covers_the_stated_inputs():
    assert {"f32", "f64", "const", "extremes"} <= set(GOLD_INPUTS)
    assert GOLD["in_f32"].dtype == np.float32 and GOLD["in_f64"].dtype == np.float64
    assert np.ptp(GOLD["in_const"]) == 0
    x = GOLD["in_extremes"]
    assert (x == x.min()).sum() > 1 and (x == x.max()).sum() > 1


@pytest.mark.parametrize("key", GOLD_INPUTS)
def test_index_and_table_stage_equals_matplotlib(key):
    x = GOLD["in_" + key]
    for name in ("jet", "gray"):
        got = ref.colorize(x, GOLD["table_" + name])
        assert np.array_equal(got, GOLD["out_%s_%s" % (key, name)]), (key, name)
    if key == "const":
        assert not ref.lut_index(x).any()


# ---- the whole rule, by hand -----------------------------------------------------------------------------------------
JET, GRAY = GOLD["table_jet"], GOLD["table_gray"]


def test_constant_frame_and_map_give_index_zero():
    frame = np.full((224, 298, 3), 0.4, np.float32)
    energy = np.zeros((36, 48), np.float32)
    assert np.ptp(ref.grey(frame)) == 0 and np.ptp(ref.resize_map(energy)) == 0
    out = ref.render(frame, energy, GRAY, JET)
    # gray[0] = (0, 0, 0), jet[0] = (0, 0, 127): (7 * 127 + 3 * 0 + 5) // 10 = 89
    assert tuple(JET[0]) == (0, 0, 127) and tuple(GRAY[0]) == (0, 0, 0)
    assert out.shape == (224, 298, 3) and out.dtype == np.uint8
    assert (out == np.array([0, 0, 89], np.uint8)).all()
    # a flat layer is one whose VALUES are equal after the resize.  The float32 weights (1 - f, f) do not always sum to
    # one (1 - f rounds where f has more digits than 1 - f can hold), so a non-zero constant map comes out of cv2.resize
    # with last-place noise, which the autoscale then spreads over the whole table - in the reference's figures too
    noisy = ref.resize_map(np.full((36, 48), 0.0415, np.float32))
    assert 0 < np.ptp(noisy) < 1e-8 and ref.lut_index(noisy).max() == 255


def test_alpha_zero_is_the_base_and_alpha_one_the_overlay():
    rng = np.random.RandomState(3)
    frame = rng.rand(224, 298, 3).astype(np.float32)
    energy = rng.rand(36, 48).astype(np.float32)
    base = ref.colorize(ref.grey(frame), GRAY)
    over = ref.colorize(ref.resize_map(energy), JET)
    assert np.array_equal(ref.render(frame, energy, GRAY, JET, alpha=(0, 10)), base)
    assert np.array_equal(ref.render(frame, energy, GRAY, JET, alpha=(10, 10)), over)
    # one pixel of the 7 / 10 blend by hand
    want = [(7 * int(over[100, 100, c]) + 3 * int(base[100, 100, c]) + 5) // 10 for c in range(3)]
    assert ref.render(frame, energy, GRAY, JET)[100, 100].tolist() == want


def test_grey_is_the_stated_float32_expression():
    f = np.array([[[0.3, 0.6, 0.9]]], np.float32)
    a = np.float32(np.float32(0.3) * np.float32(0.114))
    b = np.float32(np.float32(0.6) * np.float32(0.587))
    c = np.float32(np.float32(0.9) * np.float32(0.299))
    assert ref.grey(f)[0, 0] == np.float32(np.float32(a + b) + c)


def test_two_valued_map_extremes_on_border_columns():
    """only source column 0 holds the minimum and only column 47 the maximum: the border clamp (f = 0) carries both to
    the frame's edge columns, so they index entries 0 and 255; 2.51 in between is t = 0.3775 -> entry 96"""
    energy = np.full((36, 48), 2.51, np.float32)
    energy[:, 0], energy[:, 47] = 1.0, 5.0
    v = ref.resize_map(energy)
    # rows 0 and 223 clamp too (weights 1, 0): exact there; elsewhere the weights' sum may miss one by a last place
    assert v[0, 0] == 1.0 and v[223, 0] == 1.0 and v[0, 297] == 5.0 and v[223, 297] == 5.0
    assert np.abs(v[:, :3] - 1.0).max() < 1e-6 and np.abs(v[:, 295:] - 5.0).max() < 1e-6
    assert np.argmin(v) % 298 < 3 and np.argmax(v) % 298 >= 295
    frame = np.zeros((224, 298, 3), np.float32)
    out = ref.render(frame, energy, GRAY, JET, alpha=(10, 10))
    assert (out[:, 0] == JET[0]).all() and (out[:, 297] == JET[255]).all() and (out[:, 150] == JET[96]).all()


def test_outline_rule():
    m = ref.outline_mask(boxes_of((10, 20, 30, 40)))
    # outer 13 x 13 (9..21, 29..41) minus inner 7 x 7 (12..18, 32..38)
    assert m.sum() == 13 * 13 - 7 * 7
    assert m[29, 9] and m[41, 21] and m[31, 11] and not m[32, 12] and not m[28, 9] and not m[35, 15] and m[35, 19]
    # reversed corners: the same outline
    assert np.array_equal(ref.outline_mask(boxes_of((20, 10, 40, 30))), m)
    # xmax == 0: absent, whatever the other fields hold
    assert not ref.outline_mask(boxes_of((10, 0, 30, 40))).any()
    # off the frame entirely; partly: outer (0..6)^2 minus inner (0..3)^2
    assert not ref.outline_mask(boxes_of((-30, -5, 30, 40))).any()
    assert not ref.outline_mask(boxes_of((310, 400, 30, 40))).any()
    assert ref.outline_mask(boxes_of((-10, 5, -10, 5))).sum() == 49 - 16
    # narrower than 4 pixels: no interior, the 5 x 13 block is solid
    n = ref.outline_mask(boxes_of((50, 52, 30, 40)))
    assert n.sum() == 5 * 13 and n[29:42, 49:54].all()
    # three annotators: the union
    u = ref.outline_mask(boxes_of((10, 20, 30, 40), (50, 52, 30, 40), (10, 0, 0, 200)))
    assert np.array_equal(u, m | n)


def test_outline_pixels_take_the_top_grey_entry():
    frame = np.full((224, 298, 3), 0.25, np.float32)
    frame[0, 0] = 0.0                                     # grey range [0, 0.25] without boxes, [0, 1] with
    energy = np.full((36, 48), 1.0, np.float32)
    b = boxes_of((10, 20, 30, 40))
    out = ref.render(frame, energy, GRAY, JET, boxes=b, alpha=(0, 10))
    m = ref.outline_mask(b)
    assert (out[m] == GRAY[255]).all() and (out[0, 0] == GRAY[0]).all()
    g = np.float32(np.float32(np.float32(0.25) * np.float32(0.114) + np.float32(0.25) * np.float32(0.587))
                   + np.float32(0.25) * np.float32(0.299))
    assert (out[~m][1:] == GRAY[int(g * 256)]).all()
    assert (ref.render(frame, energy, GRAY, JET, alpha=(0, 10))[100, 100] == GRAY[255]).all()


# ---- PNG -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (224, 298), (5, 7), (224, 604)])
def test_write_png_round_trip(tmp_path, shape):
    from acimg.png import write_png
    rng = np.random.RandomState(shape[1])
    img = rng.randint(0, 256, size=shape + (3,)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    n = write_png(path, img, level=3)
    with open(path, "rb") as f:
        data = f.read()
    assert n == len(data)
    assert np.array_equal(read_png(data), img)
    # a view (one panel of a wider canvas) is written as its pixels, not as its memory
    if shape[1] > 2:
        write_png(path, img[:, 1:-1], level=1)
        with open(path, "rb") as f:
            assert np.array_equal(read_png(f.read()), img[:, 1:-1])


def test_write_png_refuses_other_layouts(tmp_path):
    from acimg.png import write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32),
                np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "b.png"), bad)


def test_write_png_agrees_with_pil(tmp_path):
    from acimg.png import write_png
    img = np.random.RandomState(9).randint(0, 256, size=(33, 61, 3)).astype(np.uint8)
    path = str(tmp_path / "c.png")
    write_png(path, img)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (61, 33)
        assert np.array_equal(np.asarray(im), img)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_show_arguments_directories_and_names(tmp_path):
    from acimg import show
    v = show.parse_args(["video", "--train_file", "/data/set/class_5/video_12/testing.txt", "--init_checkpoint",
                         "/runs/a b/epoch_41.ckpt"])
    assert (v.command, v.model, v.batch_size, v.sample_length, v.data_type) == ("video", "UNet", 2, 1, "outdoor")
    assert show.output_dir(v) == "/data/set/class_5/video_12/Generated_10s"
    assert show.frame_file(v, 7) == "/data/set/class_5/video_12/Generated_10s/I_000007.png"
    track, merge = show.ffmpeg_commands(v)
    assert track == ("ffmpeg -y -r 12 -f image2 -s 640x480 -i /data/set/class_5/video_12/Generated_10s/I_%06d.png "
                     "-vcodec libx264 -crf 25 -pix_fmt yuv420p /data/set/class_5/video_12/video_track.avi")
    assert merge == ("ffmpeg -y -i /data/set/class_5/video_12/audio/output_audio2.wav -i "
                     "/data/set/class_5/video_12/video_track.avi -codec copy -shortest "
                     "/data/set/class_5/video_12/video_razor_video_12_41.avi")

    i = show.parse_args(["images", "--model", "UNet", "--datatype", "outdoor", "--train_file", "/lists/testing.txt",
                         "--init_checkpoint", "/runs/x/epoch_41.ckpt", "--batch_size", "4", "--nr_frames", "1"])
    assert show.output_dir(i) == "/runs/x/UNet_testing_AcousticMapJet_41"
    assert show.frame_file(i, 0) == "/runs/x/UNet_testing_AcousticMapJet_41/testing_images_0.png"

    b = show.parse_args(["boxes", "--train_file", "/lists/flickr_test.txt", "--init_checkpoint", "/runs/x/epoch_9.ckpt",
                         "--plot", "1", "--threshold", "0.5", "--num_skip_conn", "2", "--ae", "1"])
    assert (b.datatype, b.num_skip_conn, b.ae) == ("frames", 2, 1)
    assert show.output_dir(b) == "/runs/x/UNet_flickr_test_AcousticFramesJet2_9"
    assert show.frame_file(b, 123) == "/runs/x/UNet_flickr_test_AcousticFramesJet2_9/flickr_test_images_123.png"
    # the same directory acimg.localize scores into
    from acimg import localize
    la = localize.parse_args(["--train_file", "/lists/flickr_test.txt", "--init_checkpoint", "/runs/x/epoch_9.ckpt"])
    assert localize.output_dir(la) == show.output_dir(b)

    for bad in ([], ["movie"], ["video"], ["video", "--train_file", "x"]):
        with pytest.raises(SystemExit):
            show.parse_args(bad)

    # show.json
    lst = tmp_path / "class_1" / "video_3" / "testing.txt"
    lst.parent.mkdir(parents=True)
    v = show.parse_args(["video", "--train_file", str(lst), "--init_checkpoint", str(tmp_path / "epoch_5.ckpt")])
    os.makedirs(show.output_dir(v))
    res = show.write_summary(v, 24, 298)
    with open(os.path.join(show.output_dir(v), show.RESULT_FILE)) as f:
        js = json.load(f)
    assert js == res
    assert js["num_frames"] == 24 and js["fps"] == 12 and js["printf_pattern"] == "I_%06d.png"
    assert js["file_pattern"].format(3) == "I_000003.png" and (js["height"], js["width"]) == (224, 298)
    assert js["ffmpeg"] == show.ffmpeg_commands(v) and js["ffmpeg"][1].endswith("/video_boat_video_3_5.avi")


def test_package_imports_no_plotting_library():
    pkg = os.path.join(os.path.dirname(HERE), "acoustic-image-generation_amd", "acimg")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                for line in f:
                    s = line.strip()
                    if s.startswith(("import ", "from ")):
                        assert not any(s.split()[1].split(".")[0] == m for m in ("matplotlib", "PIL", "cv2", "imageio")), \
                            (name, s)


# ---- C ABI: query and refusals, no GPU -------------------------------------------------------------------------------
def test_overlay_render_workspace_and_refusals(lib):
    import ctypes as C

    from acimg import _lib, ops
    import torch

    q = [lib.acimg_overlay_render_workspace(n) for n in (1, 7, 64)]
    assert 0 < q[0] < q[1] < q[2] and lib.acimg_overlay_render_workspace(0) == 0
    # the wrapper requires the query's bytes of its plan's workspace
    plan = ops.Plan(torch.device("cpu"))
    t = torch.zeros(64)
    ops.overlay_render(plan, t, 3, t, None, t, t, 7, 10, t, 894, 224 * 894, 64)
    assert len(plan.calls) == 1 and plan.ws.need >= q[2] > 256

    big = (C.c_char * 8192)()
    a = C.addressof(big) + (-C.addressof(big)) % 256
    EINVAL, EWORKSPACE = -1, -2

    def call(frames=a, ldf=3, logen=a, boxes=None, lb=a, lo=a, num=7, den=10, out=a, row=894, image=224 * 894, N=64,
             ws=a, nb=q[2]):
        return lib.acimg_overlay_render(frames, ldf, logen, boxes, lb, lo, num, den, out, row, image, N, ws, nb, None)

    assert call(nb=q[2] - 16) == EWORKSPACE and "workspace" in _lib.last_error()
    assert call(nb=0) == EWORKSPACE
    assert call(ws=None) == EINVAL and "null" in _lib.last_error()
    assert call(ws=None, nb=0) == EINVAL
    for k in ("frames", "logen", "lb", "lo", "out"):
        assert call(**{k: None}) == EINVAL, k
    assert call(ldf=2) == EINVAL and "ldf" in _lib.last_error()
    assert call(row=893) == EINVAL and "row_bytes" in _lib.last_error()
    assert call(image=223 * 894 + 893) == EINVAL and "image_bytes" in _lib.last_error()
    assert call(num=11, den=10) == EINVAL and "alpha" in _lib.last_error()
    assert call(num=0, den=0) == EINVAL and "alpha" in _lib.last_error()
    assert call(num=-1) == EINVAL and call(num=1, den=256) == EINVAL
    assert call(N=0) == EINVAL and call(N=65536, nb=1 << 30) == EINVAL
    assert call(ws=a + 4) == EINVAL and "aligned" in _lib.last_error()
