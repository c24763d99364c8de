"""The box-record converter's host side (acimg/jpeg.py: parse_jpeg, acimg/convert_boxes.py) and the two restatements its GPU
tests rest on: the JPEG decode chain (tests/jpeg_decode_ref.py) against Pillow's pixels of the committed fixture, bit for
bit; the resampler (tests/resample_ref.py) against its length rule and analytic tones; the parser's refusals and restart
intervals; box rounding, and the record's bytes.  Nothing here needs a GPU or Pillow."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import jpeg_decode_ref as jref  # noqa: E402
import jpeg_ref  # noqa: E402
import convert_boxes_support as support  # noqa: E402
import resample_ref as rref  # noqa: E402
from data_support import box_record  # noqa: E402

RATES = (22050, 44100, 48000, 8000, 11025)


@pytest.fixture(scope="module")
def golden():
    return jref.load_golden()


# ---- JPEG -------------------------------------------------------------------------------------------------------------------
EXTREME = ("blocks_444", "blocks_420", "checker_444", "checker_grey", "colour_blocks_444", "harsh_420_optimize",
           "restart1_blocks_420")


def test_fixture_holds_the_cases(golden):
    assert len(golden) == 30 + len(EXTREME) and list(golden)[30:] == list(EXTREME)
    assert list(jref.load_golden(jref.GOLDEN_FILES[:1])) == list(golden)[:30]
    infos = {n: jref.parse_stream(d) for n, (d, _) in golden.items()}
    assert {(i.comps, i.hs, i.vs) for i in infos.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {(p.shape[1], p.shape[0]) for _, p in golden.values()} >= {(1, 1), (17, 9), (16, 16), (37, 53), (40, 72), (256, 256)}
    assert infos["restart3_420_37x53"].restart == 3 and infos["restart1_420_40x72"].restart == 1
    for name in ("q5_noise_420_40x72", "q5_noise_444_17x9"):
        assert golden[name][1].min() == 0 and golden[name][1].max() == 255


def test_restatement_equals_pillow_bit_for_bit(golden):
    for name, (data, want) in golden.items():
        got = jref.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d of %d bytes differ" % (
            name, int((got != want).sum()), want.size)


def test_fixture_streams_reach_the_ends_of_the_format(golden):
    """what the streams make the entropy decoder, the predictor and the IDCT see, counted by the restatement's walk: DC
    differences of category 11 and AC magnitudes of size 10 (the most that 8-bit input gives), a DC coefficient of 1024,
    16-bit AC codes, DC codes beyond the 8-bit look-up, a restart after every MCU while the DC swings from end to end.  The
    floors are what full-swing images reach at quality 100 (|DC| 1024, |AC| 838); each condition names its stream."""
    reached = {}
    for name, (data, _) in golden.items():
        reached[name] = {}
        assert jref.entropy(jref.parse_stream(data), reached=reached[name])[1] == 0
    keys = ("dc_category", "ac_size", "dc_abs", "ac_abs", "dc_code_bits", "ac_code_bits")
    print()
    for title, names in (("before", list(golden)[:30]), ("after", list(golden))):
        print("%-7s" % title + "  ".join("%s %d" % (k, max(reached[n][k] for n in names)) for k in keys))
    top = {k: max(r[k] for r in reached.values()) for k in keys}
    assert top["dc_category"] == 11 and top["ac_size"] == 10 and top["dc_abs"] >= 1023 and top["ac_abs"] >= 800
    assert top["ac_code_bits"] == 16 and top["dc_code_bits"] >= 9
    for name in ("blocks_444", "blocks_420", "restart1_blocks_420"):
        assert reached[name]["dc_category"] == 11 and reached[name]["dc_abs"] == 1024 and reached[name]["dc_code_bits"] >= 9, name
    for name in ("checker_444", "checker_grey"):
        assert reached[name]["ac_size"] == 10 and reached[name]["ac_abs"] >= 800 and reached[name]["ac_code_bits"] == 16, name
    r = reached["colour_blocks_444"]
    assert (r["dc_category"], r["dc_code_bits"], r["ac_code_bits"]) == (11, 11, 16) and r["ac_size"] >= 9
    info = jref.parse_stream(golden["restart1_blocks_420"][0])
    assert info.restart == 1 and info.mcus == 24 and len(jref.entropy(info)[2]) == 24          # 23 markers: two wraps past RST7
    own, standard = (jref.parse_stream(golden[n][0]) for n in ("harsh_420_optimize", "blocks_420"))
    assert not np.array_equal(own.ac[0], standard.ac[0])                                        # its own Huffman tables
    for name in EXTREME:
        assert golden[name][1].min() == 0 and golden[name][1].max() == 255, name


@pytest.mark.parametrize("H,W,full", jpeg_ref.ENCODER_SCANS)
def test_restatement_decodes_the_encoders_scans_to_their_coefficients(H, W, full):
    files, want = jpeg_ref.encoder_files(H, W, full)
    if full:
        assert np.abs(want[..., 1:]).min() == 1023 and want[..., 0].min() == -1024
    for k, data in enumerate(files):
        info = jref.parse_stream(data)
        assert (info.height, info.width, info.hs, info.vs, info.mcus, info.blocks) == (H, W, 2, 2, want.shape[1], 6)
        reached = {}
        coef, status, offsets = jref.entropy(info, reached=reached)
        assert status == 0 and coef.shape == want[k].shape and np.array_equal(coef, want[k]), (H, W, full, k)
        assert len(offsets) == (1 if k == 0 else -(-info.mcus // info.restart))
        if full:
            assert (reached["dc_category"], reached["ac_size"], reached["ac_abs"], reached["ac_code_bits"]) == (11, 10, 1023, 16)


def test_parser_agrees_with_the_restatement(golden):
    """geometry, quant tables, the scan's range, and the restart offsets the byte search finds against those the
    restatement meets while it walks the scan"""
    from acimg import jpeg
    for name, (data, _) in golden.items():
        info, r = jpeg.parse_jpeg(data, name), jref.parse_stream(data)
        coef, status, offsets = jref.entropy(r)
        assert status == 0
        assert (info.height, info.width, info.comps, info.hs, info.vs) == (r.height, r.width, r.comps, r.hs, r.vs)
        assert (info.mcu_w, info.mcu_h, info.mcus, info.blocks) == (r.mcu_w, r.mcu_h, r.mcus, r.blocks)
        assert (info.scan_begin, info.scan_end) == (r.scan_begin, len(data) - 2), name
        assert info.restart_mcus == r.restart
        assert all(np.array_equal(info.quant[c], r.quant[c]) for c in range(r.comps))
        assert info.intervals[:, 0].tolist() == offsets, name
        assert info.intervals[1:, 0].tolist() == (info.intervals[:-1, 1] + 2).tolist()
        assert info.intervals[-1, 1] == info.scan_end - info.scan_begin
    assert len(jpeg.parse_jpeg(golden["restart3_420_37x53"][0]).intervals) == 4
    assert len(jpeg.parse_jpeg(golden["restart5_420_37x53"][0]).intervals) == 3          # 5, 5 and 2 MCUs
    assert len(jpeg.parse_jpeg(golden["restart1_420_40x72"][0]).intervals) == 15


def test_derived_huffman_tables_decode_like_the_restatement(golden):
    """the device layout, read back on the host the way the kernel reads it, against the restatement's 16-bit look-up"""
    from acimg import jpeg
    for name in ("optimize_420_37x53", "noise_420_16x16", "grey_17x9"):
        data = golden[name][0]
        info, r = jpeg.parse_jpeg(data, name), jref.parse_stream(data)
        for c in range(r.comps):
            for k, want in enumerate((r.dc[c], r.ac[c])):
                t = info.huff[2 * c + k]
                look, maxcode = t[:512].view(np.uint16), t[512:580].view(np.int32)
                valoff, vals = t[580:648].view(np.int32), t[648:]
                for bits in range(0, 65536, 7):
                    e = int(look[bits >> 8])
                    if not e:
                        for length in range(9, 17):
                            code = bits >> (16 - length)
                            if code <= maxcode[length]:
                                e = (length << 8) | int(vals[(valoff[length] + code) & 255])
                                break
                    assert e == int(want[bits]), (name, c, k, bits)


def test_parser_refusals_by_name(golden):
    from acimg import jpeg
    from acimg.convert import ConvertError
    data = golden["noise_420_16x16"][0]
    sof, dqt = jref.payload_offset(data, 0xC0), jref.payload_offset(data, 0xDB)
    cases = [(jref.as_progressive(data), "progressive"),
             (data[:sof + 4], "truncated"),
             (data[:3], "not a JPEG"),
             (jref.patched(data, sof + 7, 0x12), "sampling 1x2"),
             (jref.patched(data, dqt, 0x10 | data[dqt]), "16-bit DQT"),
             (jref.patched(data, sof, 12), "12-bit"),
             (jref.patched(data, sof - 3, 0xC9), "arithmetic")]
    for bad, word in cases:
        with pytest.raises(ConvertError, match=word) as e:
            jpeg.parse_jpeg(bad, "some/dir/frame.jpg")
        assert "some/dir/frame.jpg" in str(e.value)
    # a scan that ends early is the device's to report: the parser takes it and bounds the segment by the file
    cut = data[:jpeg.parse_jpeg(data).scan_begin + 20]
    info = jpeg.parse_jpeg(cut)
    assert info.scan_end == len(cut)
    r = jref.parse_stream(cut)
    assert jref.entropy(r)[1] != 0


# ---- resampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_resampled_length_rule(rate):
    from acimg import convert_boxes as cb
    for n in (1, 50, 3000):
        ratio = 12288.0 / rate
        formed, returned = int(n * ratio), int(np.ceil(n * ratio))
        assert rref.lengths(n, rate) == (formed, returned) == cb.resampled_length(n, rate)
        x = np.random.RandomState(n).randint(-3000, 3000, size=n)
        y = rref.resample_f64(x, rate)
        assert y.shape == (returned,) and not y[formed:].any()
        assert rref.resample(x, rate).dtype == np.int32


def test_pass_through_at_12288():
    x = np.random.RandomState(0).randint(-2 ** 31, 2 ** 31, size=777).astype(np.int32)
    assert np.array_equal(rref.resample(x, 12288), x)


def test_product_and_restatement_build_the_same_filter():
    from acimg import convert_boxes as cb
    for rate in RATES:
        ratio = 12288.0 / rate
        a, b = cb.sinc_window(ratio), rref.sinc_window(ratio)
        assert a[2] == b[2] == 512 and a[0].shape == (32769,)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[1][-1] == 0 and a[0][0] == min(1.0, ratio) * rref.ROLLOFF


# worst |restatement - analytic tone| / amplitude over the interior samples, measured with this restatement on 3000
# samples of a 440 Hz and a 1500 Hz tone (the larger of the two): 6.1e-7 at 8000 Hz, 3.8e-7 at 11025 Hz, 6.7e-4 at 22050 Hz,
# 3.6e-3 at 44100 Hz, 4.3e-4 at 48000 Hz.  The bounds are twice the figures the definition was checked to: 1e-6 when
# upsampling, 6.7e-4, 3.6e-3 and 4.3e-4.  When downsampling nearly all of the error is a GAIN: resampy steps through the
# table by int(scale * 512) entries where scale * 512 is 285.3, 142.7 and 131.1, so the taps lie denser than the filter was
# scaled for.  The fitted gain is 1 + 5.8e-4, 1 + 3.5e-3 and 1 + 4.3e-4 (the table steps alone would give 1.1e-3, 4.7e-3
# and 5.5e-4; the roll-off takes some back), and what is left after it is 2.4e-4, 5.0e-4 and 5.4e-5.  That gain is the
# reference's behaviour and is kept.
TONE_BOUND = {8000: 2e-6, 11025: 2e-6, 22050: 2 * 6.7e-4, 44100: 2 * 3.6e-3, 48000: 2 * 4.3e-4}


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("tone", (440.0, 1500.0))
def test_tone_against_the_analytic_tone(rate, tone):
    amplitude, n = 20000.0, 3000
    x = amplitude * np.sin(2 * np.pi * tone * np.arange(n) / rate)
    y = rref.resample_f64(x, rate)
    ratio = 12288.0 / rate
    edge = int(64 * max(1.0, ratio)) + 2                   # the filter's 64 zero crossings, in output samples
    inner = slice(edge, rref.lengths(n, rate)[0] - edge)
    want = amplitude * np.sin(2 * np.pi * tone * np.arange(y.size) / 12288.0)
    err = float(np.abs(y[inner] - want[inner]).max() / amplitude)
    print("%d Hz, %g Hz tone: worst interior error %.3e of the amplitude (bound %.1e)" % (rate, tone, err, TONE_BOUND[rate]))
    assert y[inner].size > 500 and err <= TONE_BOUND[rate]


# ---- boxes and the record ---------------------------------------------------------------------------------------------------
def test_box_rounding_and_typescene():
    from acimg import convert_boxes as cb
    from acimg.convert import ConvertError
    # 64 * 298 / 256 = 74.5 -> 74 (half to even); 4 * 224 / 256 = 3.5 -> 4; 12 * 224 / 256 = 10.5 -> 10; 192 * 298 / 256 = 223.5 -> 224
    assert [cb.scale_box(v, 298) for v in (0, 64, 192, 100, 256)] == [0, 74, 224, 116, 298]
    assert [cb.scale_box(v, 224) for v in (4, 12, 100, 256)] == [4, 10, 88, 224]
    for v in range(0, 600, 7):
        assert cb.scale_box(v, 298) == int(np.round(v * 298 / 256)) and cb.scale_box(v, 224) == int(np.round(v * 224 / 256))
    persons = [("object", 64, 4, 192, 12), ("ambient sound", 10, 20, 30, 40)]
    boxes, scene = cb.parse_annotation(support.annotation_xml("77", persons), "77", "a/77.xml")
    assert boxes.dtype == np.int32 and scene.dtype == np.int32
    assert boxes.tolist() == [[74, 12, 0], [224, 35, 0], [4, 18, 0], [10, 35, 0]] and scene.tolist() == [1, 0, 0]
    boxes, scene = cb.parse_annotation(support.annotation_xml("77", []), "77")
    assert not boxes.any() and not scene.any()
    three = [("object", 1, 2, 3, 4)] * 3
    assert cb.parse_annotation(support.annotation_xml("77", three), "77")[1].tolist() == [1, 1, 1]
    with pytest.raises(ConvertError, match=r"a/77\.xml: 4 person entries"):
        cb.parse_annotation(support.annotation_xml("77", three + three[:1]), "77", "a/77.xml")
    with pytest.raises(ConvertError, match=r"a/77\.xml: file_name '78\.jpg'"):
        cb.parse_annotation(support.annotation_xml("77", three, file_name="78.jpg"), "77", "a/77.xml")
    with pytest.raises(ConvertError, match="no XML"):
        cb.parse_annotation(b"<annotation>", "77")


def test_record_bytes_equal_the_test_helper():
    from acimg import convert_boxes as cb
    from acimg import tfio
    rng = np.random.RandomState(3)
    boxes = rng.randint(0, 298, size=(4, 3)).astype(np.int32)
    scene = np.array([1, 0, 1], np.int32)
    audio = rng.randint(-2 ** 31, 2 ** 31, size=5571).astype(np.int32)
    video = rng.randint(0, 256, size=(224, 298, 3)).astype(np.uint8)
    rec = cb.build_box_record(boxes, scene, audio, video)
    assert rec == box_record(boxes, scene, audio, video)
    d = tfio.decode_box_sequence_example_native(rec)
    assert np.array_equal(d["boxes"][0], boxes) and np.array_equal(d["typescene"][0], scene)
    assert np.array_equal(d["audio_samples"].reshape(-1), audio) and np.array_equal(d["video_images"][0], video)
    assert cb.build_box_record(boxes, scene, None, video) == box_record(
        boxes, scene, audio, video, drop=("audio_data/mics", "audio_data/samples", "audio/data"))


def test_walk_and_its_refusals(tmp_path):
    from acimg import convert_boxes as cb
    from acimg.convert import ConvertError
    root = tmp_path / "raw"
    for fold, names in (("1", ("5.jpg", "3.jpg", "9.jpg", "3.wav")), ("0", ("7.jpg",))):
        d = root / "Dataset" / "Data" / fold
        d.mkdir(parents=True)
        for n in names:
            (d / n).write_bytes(b"")
    with pytest.raises(ConvertError, match="test_list.txt"):
        cb.find_files(str(root), "/out")
    (root / "test_list.txt").write_text("3.jpg\n7.jpg\n5.jpg\n")
    items = cb.find_files(str(root), "/out")
    assert [i.ident for i in items] == ["7", "3", "5"]
    assert items[1].wav == str(root / "Dataset" / "Data" / "1" / "3.wav") and items[1].out == "/out/3.tfrecord"
    assert items[1].xml == str(root / "Dataset" / "Annotations" / "3.xml")
    (root / "test_list.txt").write_text("3.jpg\n8.jpg\n")
    with pytest.raises(ConvertError, match=r"8\.jpg"):
        cb.find_files(str(root), "/out")
