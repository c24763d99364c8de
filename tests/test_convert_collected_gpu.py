"""`python -m acimg.convert_collected` end to end on a tree of writer-made PNGs (one interlaced 16-bit, one palette, one of
another size) and short WAVs at three rates, with `--deflate` and `--inflate` at both values; read back through
`ClassRecordLoader` and held to the samples the PNGs were written from, to the restatement (tests/png_decode_ref.py) and
to the resampler's restatement (tests/resample_ref.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import convert_collected_support as support  # noqa: E402
import png_decode_ref as ref  # noqa: E402
import png_writer  # noqa: E402
import resample_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER = (1, 7, 12, 23)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    raw = tmp_path_factory.mktemp("collected")
    return raw, support.write_tree(raw)


@pytest.fixture(scope="module")
def converted(device, tree, tmp_path_factory):
    """(deflate, inflate) -> (out dir, list file, what the CLI printed) for the four combinations"""
    import contextlib
    import io

    from acimg import convert_collected as cc
    raw, _ = tree
    runs = {}
    for deflate in ("zlib", "device"):
        for inflate in ("zlib", "device"):
            out = tmp_path_factory.mktemp("out_%s_%s" % (deflate, inflate))
            lst = str(out) + ".txt"
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                assert cc.main([str(raw), str(out), "--device", str(device), "--workers", "3", "--deflate", deflate,
                                "--inflate", inflate, "--list", lst]) == 0
            runs[(deflate, inflate)] = (out, lst, text.getvalue())
    return runs


def test_records_hold_the_pngs_pixels_and_the_resampled_clips(tree, converted):
    from acimg import tfio
    raw, want = tree
    out, lst, printed = converted[("zlib", "zlib")]
    assert open(lst).read() == "".join("%s/%s\n" % (out, n.replace(".png", ".tfrecord")) for n in support.LISTED)
    assert sorted(os.listdir(str(out))) == sorted("%d.tfrecord" % i for i in ORDER)
    assert "\n53 37 3\n" in printed and "298 224" not in printed                # only the other size is printed, as there
    assert "4 records; seconds in read" in printed
    for ident in ORDER:
        path = "%s/%d.tfrecord" % (out, ident)
        with open(path, "rb") as f:
            assert f.read(2) == b"\x1f\x8b"                                     # GZIP
        (rec,) = list(tfio.read_tfrecord(path))
        ctx, lists = tfio.parse_sequence_example(rec)
        bgr, sound = want[ident]
        clip = rref.resample(sound, support.RECORDINGS[ident][1][0])
        values = {k: int(np.asarray(v).reshape(-1)[0]) for k, v in ctx.items()}
        assert values == {"audio_data/mics": 1, "audio_data/samples": clip.size, "classnumber": support.CLASS_OF_ID[ident - 1],
                          "video/height": bgr.shape[0], "video/width": bgr.shape[1], "video/depth": 3}, ident
        assert lists["audio/data"] == [[clip.astype("<i4").tobytes()]], ident
        assert lists["video/image"] == [[bgr.tobytes()]], ident
    for ident in (12, 23):                                                      # and the restatement says the same
        assert np.array_equal(ref.decode_png((raw / ("%d.png" % ident)).read_bytes())[1], want[ident][0])


def test_class_record_loader_reads_the_converted_set(tree, converted):
    from acimg.data import ClassRecordLoader, box_mfcc
    _, want = tree
    out = converted[("device", "device")][0]
    ids = (7, 23, 1)                                                            # the three of the data set's size
    (batch,) = list(ClassRecordLoader(["%s/%d.tfrecord" % (out, i) for i in ids], 3))
    assert not batch[0].any() and tuple(batch[0].shape) == (3, 36, 48, 12)
    frames = np.stack([want[i][0][..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0) for i in ids])
    assert np.array_equal(batch[2].numpy(), frames)
    clips = [rref.resample(want[i][1], support.RECORDINGS[i][1][0]) for i in ids]
    assert np.array_equal(batch[1].numpy(), np.concatenate([box_mfcc(c[None]) for c in clips]))
    assert batch[3].tolist() == [[2], [5], [9]]
    with pytest.raises(ValueError, match=r"12.tfrecord: a frame of 37 x 53 x 3"):
        list(ClassRecordLoader(["%s/12.tfrecord" % out], 1))


def test_inflate_modes_write_the_same_bytes_and_deflate_modes_the_same_records(converted):
    from acimg import tfio
    for deflate in ("zlib", "device"):
        a, b = converted[(deflate, "zlib")][0], converted[(deflate, "device")][0]
        for ident in ORDER:
            assert (a / ("%d.tfrecord" % ident)).read_bytes() == (b / ("%d.tfrecord" % ident)).read_bytes(), (deflate, ident)
    a, b = converted[("zlib", "zlib")][0], converted[("device", "zlib")][0]
    for ident in ORDER:
        ra, rb = (list(tfio.read_tfrecord(str(d / ("%d.tfrecord" % ident)))) for d in (a, b))
        assert len(ra) == 1 and ra == rb, ident


def test_a_corrupt_png_is_refused_before_a_byte_of_its_batch_is_written(device, tree, tmp_path):
    """a filter byte of 5 is found on the device, after the decode; a flipped CRC bit on the host, before it"""
    from acimg import convert_collected as cc
    from acimg.convert import ConvertError
    src, _ = tree
    raw, out = tmp_path / "raw", tmp_path / "out"
    raw.mkdir()
    out.mkdir()
    for name in ("7.png", "7.wav", "12.wav"):
        (raw / name).write_bytes((src / name).read_bytes())
    (raw / "12.png").write_bytes(png_writer.write_png(np.zeros((5, 4, 3), np.uint16), 2, 8, (0, 1, 5, 2, 0)))
    (raw / "test_list.txt").write_text("12.png\n7.png\n")
    lst = str(tmp_path / "list.txt")
    for inflate in ("zlib", "device"):
        with pytest.raises(ConvertError, match=r"12\.png: corrupt PNG: a filter byte above 4"):
            cc.main([str(raw), str(out), "--device", str(device), "--inflate", inflate, "--list", lst])
        assert os.listdir(str(out)) == [] and not os.path.exists(lst)
    good = (src / "12.png").read_bytes()
    at = good.index(b"IDAT") + 9
    (raw / "12.png").write_bytes(good[:at] + bytes([good[at] ^ 4]) + good[at + 1:])
    with pytest.raises(ConvertError, match=r"12\.png: CRC mismatch in chunk IDAT"):
        cc.main([str(raw), str(out), "--device", str(device), "--list", lst])
    assert os.listdir(str(out)) == [] and not os.path.exists(lst)
