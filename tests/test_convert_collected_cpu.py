"""The two-object test-set converter's host side (acimg/convert_collected.py) on fake trees: the walk, the label table,
the refusals (each before a byte is written), the record's bytes and the list file; `acimg.data.ClassRecordLoader` on
records built with `tfio`.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import convert_collected_support as support  # noqa: E402
import convert_ref  # noqa: E402


@pytest.fixture()
def tree(tmp_path):
    raw, out = tmp_path / "raw", tmp_path / "out"
    raw.mkdir()
    out.mkdir()
    return raw, out, support.write_tree(raw)


def test_label_table():
    from acimg import convert_collected as cc
    from acimg.convert import ConvertError
    assert cc.CLASS_OF_ID == support.CLASS_OF_ID and len(cc.CLASS_OF_ID) == 23 and len(cc.CLASS_NAMES) == 10
    assert max(cc.CLASS_OF_ID) == len(cc.CLASS_NAMES) - 1
    assert [cc.class_of(i) for i in (1, 7, 20, 23)] == [9, 2, 0, 5]
    for ident in (0, 24, -1):
        with pytest.raises(ConvertError, match=r"x.png: id %d has no class: the table holds ids 1 .. 23" % ident):
            cc.class_of(ident, "x.png")


def test_walk_is_sorted_by_integer_id(tree):
    from acimg import convert_collected as cc
    raw, out, _ = tree
    (raw / "3.png").write_bytes(b"not listed")
    items, listed = cc.find_files(str(raw), str(out))
    assert listed == list(support.LISTED)
    assert [i.ident for i in items] == [1, 7, 12, 23]                       # not '1', '12', '23', '7'
    assert [i.classnumber for i in items] == [9, 2, 7, 5]
    assert items[2] == cc.Item(12, str(raw / "12.png"), str(raw / "12.wav"), "%s/12.tfrecord" % out, 7)


@pytest.mark.parametrize("listed,text", [
    (("7.png", "9.png"), r"test_list.txt: 2 file\(s\) of the listed recordings are not in .*, the first is 9.png"),
    (("7.png", "007.png"), r"test_list.txt: '007.png' is not <id>.png with the id in canonical decimal form"),
    (("7.png", "seven.png"), r"'seven.png' is not <id>.png"),
    (("7.png", "7.jpg"), r"'7.jpg' is not <id>.png"),
    (("7.png", "+7.png"), r"'\+7.png' is not <id>.png"),
    (("7.png", "0.png"), r"0.png: id 0 has no class"),
    (("7.png", "24.png"), r"24.png: id 24 has no class"),
])
def test_refused_before_a_byte_is_written(tree, listed, text):
    from acimg import convert_collected as cc
    from acimg.convert import ConvertError
    raw, out, _ = tree
    (raw / "test_list.txt").write_text("".join(n + "\n" for n in listed))
    with pytest.raises(ConvertError, match=text):
        cc.convert(str(raw), str(out), modalities=[0], device="cpu")
    assert os.listdir(str(out)) == [] and not (raw / "test.txt").exists()


def test_a_missing_wav_and_a_missing_list_are_refused(tree):
    from acimg import convert_collected as cc
    from acimg.convert import ConvertError
    raw, out, _ = tree
    os.remove(str(raw / "23.wav"))
    with pytest.raises(ConvertError, match=r"the first is 23.wav"):
        cc.find_files(str(raw), str(out))
    os.remove(str(raw / "test_list.txt"))
    with pytest.raises(ConvertError, match=r"test_list.txt: the list of files to convert cannot be read"):
        cc.find_files(str(raw), str(out))
    with pytest.raises(ConvertError, match="--inflate is one of zlib, device"):
        cc.CollectedConverter(modalities=[0], device="cpu", inflate="host")


def test_record_bytes():
    from acimg import convert_collected as cc
    from acimg import tfio
    audio = np.array([5, -7, 2 ** 31 - 1, -2 ** 31], np.int32)
    video = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    ctx, lists = tfio.parse_sequence_example(cc.build_class_record(6, audio, video))
    assert list(ctx) == ["audio_data/mics", "audio_data/samples", "classnumber", "video/height", "video/width", "video/depth"]
    assert [int(np.asarray(v).reshape(-1)[0]) for v in ctx.values()] == [1, 4, 6, 2, 3, 3]
    assert list(lists) == ["audio/data", "video/image"]
    assert lists["audio/data"] == [[audio.astype("<i4").tobytes()]] and lists["video/image"] == [[video.tobytes()]]       # one step each
    ctx, lists = tfio.parse_sequence_example(cc.build_class_record(6, None, video))           # the label goes with the audio
    assert list(ctx) == ["video/height", "video/width", "video/depth"] and list(lists) == ["video/image"]
    ctx, lists = tfio.parse_sequence_example(cc.build_class_record(6, audio, None))
    assert list(ctx) == ["audio_data/mics", "audio_data/samples", "classnumber"] and list(lists) == ["audio/data"]


def test_list_file_follows_test_list(tree, tmp_path):
    """without a modality nothing touches the device: the records are empty, the list is the reference's"""
    from acimg import convert_collected as cc
    from acimg import tfio
    raw, out, _ = tree
    paths, conv = cc.convert(str(raw), str(out), modalities=[0], device="cpu")
    assert paths == ["%s/%d.tfrecord" % (out, i) for i in (1, 7, 12, 23)] and conv.records == 4
    assert (raw / "test.txt").read_text() == "".join("%s/%s\n" % (out, n.replace(".png", ".tfrecord")) for n in support.LISTED)
    assert sorted(os.listdir(str(out))) == sorted("%d.tfrecord" % i for i in (1, 7, 12, 23))
    (rec,) = list(tfio.read_tfrecord(paths[0]))
    assert tfio.parse_sequence_example(rec) == ({}, {})
    lst = tmp_path / "list.txt"
    assert cc.main([str(raw), str(out), "--modalities", "0", "--device", "cpu", "--list", str(lst)]) == 0
    assert lst.read_text() == (raw / "test.txt").read_text()


# ---- ClassRecordLoader ------------------------------------------------------------------------------------------------------
def write_records(tmp_path, n, shape=(224, 298, 3)):
    from acimg import convert_collected as cc
    from acimg import tfio
    rng = np.random.RandomState(4)
    paths, want = [], []
    for k in range(n):
        audio = (rng.randn(700 + 100 * k) * 3000).astype(np.int32)
        video = rng.randint(0, 256, size=shape).astype(np.uint8)
        label = cc.CLASS_OF_ID[k]
        paths.append(str(tmp_path / ("%d.tfrecord" % (k + 1))))
        tfio.write_tfrecord(paths[-1], [cc.build_class_record(label, audio, video)], compression="GZIP")
        want.append((audio, video, label))
    return paths, want


def test_class_record_loader(tmp_path):
    from acimg.data import ClassRecordLoader, box_mfcc
    paths, want = write_records(tmp_path, 3)
    lst = tmp_path / "test.txt"
    lst.write_text("".join(p + "\n" for p in paths))
    loader = ClassRecordLoader(str(lst), 2)
    assert loader.num_samples == 3 and loader.total_batches == 2 and loader.data is loader
    batches = list(loader)
    assert [tuple(b[0].shape) for b in batches] == [(2, 36, 48, 12), (1, 36, 48, 12)] and all(len(b) == 4 for b in batches)
    ac, mfcc, video, label = [np.concatenate([b[k].numpy() for b in batches]) for k in range(4)]
    assert not ac.any() and ac.dtype == np.float32
    assert mfcc.dtype == np.float32 and np.array_equal(mfcc, np.concatenate([box_mfcc(a[None]) for a, _, _ in want]))
    assert video.dtype == np.float32 and video.shape == (3, 224, 298, 3)
    assert np.array_equal(video, np.stack([v[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0) for _, v, _ in want]))
    assert label.dtype == np.int32 and label.tolist() == [[w[2]] for w in want]
    (one,) = list(ClassRecordLoader(paths, 5))
    assert tuple(one[2].shape) == (3, 224, 298, 3) and one[3].tolist() == label.tolist()


def test_class_record_loader_refuses_another_frame_size(tmp_path):
    from acimg.data import ClassRecordLoader
    paths, _ = write_records(tmp_path, 1, shape=(37, 53, 3))
    with pytest.raises(ValueError, match=r"1.tfrecord: a frame of 37 x 53 x 3: only 224 x 298 x 3 frames are loaded"):
        list(ClassRecordLoader(paths, 1))


def test_wav_support_matches_the_converter(tmp_path):
    from acimg.convert import read_wav
    p = tmp_path / "a.wav"
    p.write_bytes(convert_ref.wav_bytes(support.sound(1), rate=44100, bits=32))
    rate, samples = read_wav(str(p))
    assert rate == 44100 and np.array_equal(samples, support.sound(1))
