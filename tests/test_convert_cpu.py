"""The dataset converter's host side (acimg/convert.py, `acimg_resize_cubic_tables`): tables against the NumPy restatement
(tests/convert_ref.py), the restatement against fp64 cubic convolution, the BMP and WAV readers, the geometry, the walk
and its refusals, and the loader's `modalities` argument.  Nothing here needs a GPU."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import convert_ref as ref  # noqa: E402


def lib_tables(n_in, n_out, first, count):
    from acimg import _lib
    idx = np.full((max(count, 1), 4), -7, np.int32)
    coef = np.full((max(count, 1), 4), -7, np.int16)
    rc = _lib.load().acimg_resize_cubic_tables(n_in, n_out, first, count, idx.ctypes.data_as(C.c_void_p),
                                               coef.ctypes.data_as(C.c_void_p))
    return rc, idx, coef


# ---- tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out,first,count", [(480, 224, 0, 224), (640, 298, 0, 298), (256, 224, 0, 224),
                                                    (37, 224, 0, 224), (300, 336, 0, 336), (1280, 398, 50, 298),
                                                    (23, 9, 2, 5)])
def test_tables_equal_the_restatement(n_in, n_out, first, count):
    rc, idx, coef = lib_tables(n_in, n_out, first, count)
    assert rc == 0
    want_idx, want_coef = ref.cubic_tables(n_in, n_out, first, count)
    assert np.array_equal(idx, want_idx) and np.array_equal(coef, want_coef)
    sums = coef.astype(np.int64).sum(1)
    assert set(sums.tolist()) <= {2047, 2048, 2049}
    assert idx.min() >= 0 and idx.max() <= n_in - 1 and (np.diff(idx, axis=1) >= 0).all()
    if first:      # a window is a slice of the whole table
        whole = ref.cubic_tables(n_in, n_out)
        assert np.array_equal(idx, whole[0][first:first + count]) and np.array_equal(coef, whole[1][first:first + count])


def test_table_sums_are_not_fixed_up():
    """2047 and 2049 occur (OpenCV leaves them): over the sizes above all three sums are seen"""
    seen = set()
    for n_in, n_out in ((480, 224), (640, 298), (37, 224), (300, 336)):
        seen |= set(ref.cubic_tables(n_in, n_out)[1].astype(np.int64).sum(1).tolist())
    assert seen == {2047, 2048, 2049}


def test_tables_refuse_arguments_out_of_range():
    from acimg import _lib
    L = _lib.load()
    for args in ((0, 224, 0, 224), (480, 0, 0, 1), (480, 224, -1, 10), (480, 224, 0, 0), (480, 224, 0, 225),
                 (480, 224, 220, 5), (480, 224, 224, 1), (65536, 224, 0, 224), (480, 65536, 0, 224)):
        rc, idx, coef = lib_tables(*args)
        assert rc == -1, args
        assert (idx == -7).all() and (coef == -7).all(), args
    idx = np.zeros((4, 4), np.int32)
    assert L.acimg_resize_cubic_tables(480, 224, 0, 4, None, idx.ctypes.data_as(C.c_void_p)) == -1
    assert L.acimg_resize_cubic_tables(480, 224, 0, 4, idx.ctypes.data_as(C.c_void_p), None) == -1
    assert "resize_cubic_tables" in _lib.last_error()


# ---- the restatement against fp64 cubic convolution ---------------------------------------------------------------------
# 0.5 from the final rounding; a weight is off by at most 0.5 / 2048, so a pass is off by at most 4 * 255 * 0.5 / 2048 =
# 0.249, and the first pass's error is carried through the second's sum |c| <= 1.27: 0.5 + 0.249 * (1 + 1.27) = 1.07.
BOUND = 1.07


@pytest.mark.parametrize("H,W,new_h,new_w", [(480, 640, 224, 298), (256, 256, 224, 224), (37, 53, 224, 320)])
def test_restatement_within_bound_of_fp64_cubic(H, W, new_h, new_w):
    rng = np.random.RandomState(H + W)
    frame = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    got = ref.resize_cubic(frame, new_h, new_w).astype(np.float64)
    err = np.abs(got - ref.resize_cubic_f64(frame, new_h, new_w)).max()
    print("%d x %d -> %d x %d: max |restatement - fp64| = %.4f levels" % (H, W, new_h, new_w, err))
    assert err <= BOUND


def test_constant_255_stays_255():
    frame = np.full((37, 53, 3), 255, np.uint8)
    for new_h, new_w in ((224, 320), (17, 20), (37, 53)):
        assert (ref.resize_cubic(frame, new_h, new_w) == 255).all()


# ---- BMP --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,bottom_up", [(64, 48, True), (64, 48, False), (53, 37, True), (53, 37, False)])
def test_bmp_parser_against_pil(W, H, bottom_up):
    from PIL import Image

    from acimg import convert
    rng = np.random.RandomState(W + bottom_up)
    bgr = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    data = ref.bmp_bytes(bgr, bottom_up=bottom_up)
    lay = convert.parse_bmp_header(data)
    pitch = (3 * W + 3) // 4 * 4
    assert (lay.height, lay.width, abs(lay.row_stride)) == (H, W, pitch) and (lay.row_stride < 0) == bottom_up
    assert lay.file_bytes <= len(data) < lay.file_bytes + 4
    got = convert.bmp_pixels(data)
    pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(got[..., ::-1], pil) and np.array_equal(got, bgr)


def test_bmp_parser_refusals():
    from acimg import convert
    bgr = np.zeros((5, 7, 3), np.uint8)
    for kw in (dict(bpp=8), dict(bpp=32), dict(bpp=8, compression=1), dict(bpp=24, compression=1)):
        with pytest.raises(convert.ConvertError, match="frame.bmp"):
            convert.parse_bmp_header(ref.bmp_bytes(bgr, **kw), "frame.bmp")
    good = ref.bmp_bytes(bgr)
    with pytest.raises(convert.ConvertError):
        convert.parse_bmp_header(b"PM" + good[2:])
    with pytest.raises(convert.ConvertError):
        convert.parse_bmp_header(good[:40])
    with pytest.raises(convert.ConvertError):
        convert.bmp_pixels(good[:-8])


def test_frame_reader_refuses_a_change_of_geometry(tmp_path):
    """the worker that reads a frame file into the staging row: same layout as the recording's first frame, or refused"""
    from acimg import convert
    rng = np.random.RandomState(9)
    files = {}
    for name, shape, up in (("first", (37, 53, 3), True), ("same", (37, 53, 3), True), ("flipped", (37, 53, 3), False),
                            ("wider", (37, 54, 3), True)):
        files[name] = str(tmp_path / (name + ".bmp"))
        with open(files[name], "wb") as f:
            f.write(ref.bmp_bytes(rng.randint(0, 256, size=shape).astype(np.uint8), bottom_up=up))
    with open(files["first"], "rb") as f:
        layout = convert.parse_bmp_header(f.read(54), files["first"])
    row = np.zeros(layout.file_bytes, np.uint8)
    convert._read_frame(files["same"], row, layout)
    with open(files["same"], "rb") as f:
        assert row.tobytes() == f.read()[:layout.file_bytes]
    for name in ("flipped", "wider"):
        with pytest.raises(convert.ConvertError, match=name + ".bmp"):
            convert._read_frame(files[name], row, layout)
    with open(files["same"], "r+b") as f:
        f.truncate(layout.file_bytes - 1)
    with pytest.raises(convert.ConvertError, match="same.bmp"):
        convert._read_frame(files["same"], row, layout)


# ---- WAV --------------------------------------------------------------------------------------------------------------------
def test_wav_reader(tmp_path):
    from acimg import convert
    rng = np.random.RandomState(3)
    for bits, lo, hi in ((16, -2 ** 15, 2 ** 15), (32, -2 ** 31, 2 ** 31)):
        x = rng.randint(lo, hi, size=2 * 12288 + 100, dtype=np.int64)
        p = str(tmp_path / ("a%d.wav" % bits))
        with open(p, "wb") as f:
            f.write(ref.wav_bytes(x, bits=bits))
        rate, got = convert.read_wav(p)
        assert rate == 12288 and got.dtype == np.int32 and np.array_equal(got, x)
        assert np.array_equal(convert.read_wav_audio_data(p, 2), x[:2 * 12288])
        with pytest.raises(convert.ConvertError, match="a%d.wav" % bits):       # short: 3 s are not there
            convert.read_wav_audio_data(p, 3)
    x = rng.randint(-100, 100, size=2 * 12288)
    for name, kw in (("stereo", dict(channels=2)), ("eight", dict(bits=8)), ("rate", dict(rate=44100))):
        p = str(tmp_path / (name + ".wav"))
        with open(p, "wb") as f:
            f.write(ref.wav_bytes(np.abs(x) if name == "eight" else x, **kw))
        with pytest.raises(convert.ConvertError, match=name + ".wav"):
            convert.read_wav_audio_data(p, 1)
    p = str(tmp_path / "junk.wav")
    with open(p, "wb") as f:
        f.write(b"RIFX" + bytes(40))
    with pytest.raises(convert.ConvertError, match="junk.wav"):
        convert.read_wav(p)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_geometry():
    from acimg import convert
    assert convert.crop_geometry(480, 640) == (224, 298, 0, 0)
    assert convert.crop_geometry(720, 1280) == (224, 398, 0, 50)
    assert convert.smallest_size_at_least(480, 640) == ref.smallest_size_at_least(480, 640) == (224, 298)
    assert convert.smallest_size_at_least(640, 480) == (298, 224)
    with pytest.raises(convert.ConvertError, match="portrait.bmp"):
        convert.crop_geometry(640, 480, "portrait.bmp")
    with pytest.raises(convert.ConvertError):
        convert.crop_geometry(480, 600)                # 224 x 280: narrower than the crop


# ---- the walk ---------------------------------------------------------------------------------------------------------------
def small_tree(root, rng):
    """class_3/data_007 (2 s), class_3/data_012 (video_time 0), class_11/data_001 (1 s): 64 x 48 frames"""
    frames = rng.randint(0, 256, size=(24, 48, 64, 3)).astype(np.uint8)
    sound = rng.randint(-2 ** 15, 2 ** 15, size=2 * 12288 + 7)
    ref.write_recording(root, 3, 7, 2, frames, sound)
    ref.write_recording(root, 3, 12, 0, frames[:1], sound)
    ref.write_recording(root, 11, 1, 1, frames[:12], sound, time_text="video time (s):  1 \n")
    return frames, sound


def test_walk_parses_class_location_and_time(tmp_path):
    from acimg import convert
    small_tree(tmp_path, np.random.RandomState(5))
    recs = convert.find_recordings(str(tmp_path))
    assert [(r.classes, r.location, r.video_time) for r in recs] == [(11, 1, 1), (3, 7, 2)]      # sorted paths; 0 s skipped
    assert recs[1].video_dir == str(tmp_path / "class_3" / "data_007" / "video")
    assert recs[1].wav == str(tmp_path / "class_3" / "data_007" / "audio" / "output_audio2.wav")
    assert convert.record_path("/out", recs[1], 2) == "/out/class_3/data_007/Data_002.tfrecord"
    (tmp_path / "class_3" / "data_007" / "video_time.txt").write_text("no colon here\n")
    with pytest.raises(convert.ConvertError, match="video_time.txt"):
        convert.find_recordings(str(tmp_path))


def test_missing_frame_is_refused_before_anything_is_written(tmp_path):
    from acimg import convert
    raw, out = tmp_path / "raw", tmp_path / "out"
    raw.mkdir()
    out.mkdir()
    small_tree(raw, np.random.RandomState(6))
    os.remove(str(raw / "class_3" / "data_007" / "video" / "I_000017.bmp"))
    conv = convert.Converter(str(out), device="cpu")
    try:
        rec = [r for r in convert.find_recordings(str(raw)) if r.location == 7][0]
        with pytest.raises(convert.ConvertError, match="I_000017.bmp"):
            conv.recording(rec)
    finally:
        conv.close()
    assert os.listdir(str(out)) == []


def test_audio_only_conversion_needs_no_device(tmp_path):
    """--modalities 1: the records hold the WAV slices and the context keys of :250-258 in order"""
    from acimg import convert, tfio
    raw, out = tmp_path / "raw", tmp_path / "out"
    raw.mkdir()
    out.mkdir()
    _, sound = small_tree(raw, np.random.RandomState(7))
    lst = str(tmp_path / "list.txt")
    paths, _ = convert.convert(str(raw), str(out), modalities=[1], list_file=lst, device="cpu", workers=2)
    want = [str(out / "class_11" / "data_001" / "Data_001.tfrecord"), str(out / "class_3" / "data_007" / "Data_001.tfrecord"),
            str(out / "class_3" / "data_007" / "Data_002.tfrecord")]
    assert paths == want and open(lst).read() == "".join(p + "\n" for p in want)
    for p, k in ((want[1], 0), (want[2], 1)):
        (rec,) = list(tfio.read_tfrecord(p))
        ctx, lists = tfio.parse_sequence_example(rec)
        assert list(ctx) == ["classes", "location", "audio_data/mics", "audio_data/samples"]
        assert [int(v[0]) for v in ctx.values()] == [3, 7, 1, 1024] and list(lists) == ["audio/data"]
        got = np.stack([np.frombuffer(s[0], "<i4") for s in lists["audio/data"]])
        assert np.array_equal(got, sound[k * 12288:(k + 1) * 12288].reshape(12, 1024))


# ---- loader ---------------------------------------------------------------------------------------------------------------
def test_loader_refuses_other_modality_subsets():
    from acimg.data import TFRecordDataLoader
    for bad in ((0, 1, 2), (1,), (2,), (0, 1), (), (1, 2, 2), (1, 3)):
        with pytest.raises(ValueError, match="modalities"):
            TFRecordDataLoader([], 4, modalities=bad)
