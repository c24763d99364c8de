"""The box-record converter on the device.  The three stages of csrc/jpeg_decode.hip through the raw C ABI, every operand
inside guard bands, against the restatement (tests/jpeg_decode_ref.py) stage by stage and against Pillow's pixels of the
committed fixture; one launch of five images whose third is corrupt; the size queries.  `acimg_resample_sinc` against
tests/resample_ref.py bit for bit, before and after the int32 conversion.  `python -m acimg.convert_boxes` end to end on a
tree written here, read back through `BoxRecordLoader`."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import convert_ref  # noqa: E402
import jpeg_decode_ref as jref  # noqa: E402
import jpeg_ref  # noqa: E402
import convert_boxes_support as support  # noqa: E402
import resample_ref as rref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B
RATES = (22050, 44100, 48000, 8000, 11025)
FIVE = ("optimize_420_37x53", "restart3_420_37x53", "noise_420_37x53", "smooth_420_37x53", "restart5_420_37x53")
FLIP_AT = 1834            # byte of noise_420_37x53's scan whose complement makes the restatement meet an unknown code


@pytest.fixture(scope="module")
def golden():
    return jref.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """name -> (coef int16 [mcus,blocks,64], planes uint8 [blocks * mcus * 64], bgr uint8 [H,W,3]); never modified"""
    out = {}
    for name, (data, _) in golden.items():
        info = jref.parse_stream(data)
        coef, status, _ = jref.entropy(info)
        assert status == 0
        planes = jref.idct(info, coef)
        arrays = (coef, np.concatenate([p.reshape(-1) for p in planes]), jref.colour(info, planes))
        for a in arrays:
            a.setflags(write=False)
        out[name] = arrays
    return out


def device_decode(device, files, what="", entropy_only=False):
    """one launch of each stage on `files` (one geometry) -> (coef, planes, bgr, status) as host arrays.  Inputs and outputs
    lie in one guard arena; the outputs are pre-filled with a sentinel and the bands are checked after every stage.
    entropy_only: the first stage alone -> (coef, status)"""
    from acimg import _lib, jpeg, ops
    L = _lib.load()
    infos = [jpeg.parse_jpeg(f, "%s[%d]" % (what, i)) for i, f in enumerate(files)]
    g, n = infos[0], len(files)
    geo = (g.height, g.width, g.comps, g.hs, g.vs)
    host = jpeg.pack_group(files, infos)
    sizes = dict(coef=n * g.mcus * g.blocks * 128, planes=n * g.mcus * g.blocks * 64, bgr=n * g.height * g.width * 3, status=4 * n)
    assert int(L.acimg_jpeg_decode_coef_bytes(n, *geo)) == sizes["coef"]
    assert int(L.acimg_jpeg_decode_plane_bytes(n, *geo)) == sizes["planes"]
    assert int(L.acimg_jpeg_decode_pixel_bytes(n, g.height, g.width)) == sizes["bgr"]
    arena = GuardArena.for_sizes(device, [a.nbytes for a in host] + list(sizes.values()))
    ins = []
    for a, name in zip(host, ("data", "desc", "intervals", "huff", "quant")):
        r = arena.region(a.nbytes, name=name)
        r.u8.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        ins.append(r)
    data, desc, intervals, huff, quant = ins
    outs = {k: arena.region(v, fill=SENT, name=k) for k, v in sizes.items()}
    st = ops.current_stream_handle(device)
    rc = L.acimg_jpeg_decode_entropy(data.ptr, host[0].nbytes, desc.ptr, intervals.ptr, host[2].shape[0], huff.ptr, n, *geo,
                                     outs["coef"].ptr, sizes["coef"], outs["status"].ptr, st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " entropy")
    if entropy_only:
        for r, a in zip(ins, host):
            assert np.array_equal(r.u8.cpu().numpy(), a.reshape(-1).view(np.uint8)), "%s: input %s was written" % (what, r.name)
        assert (outs["planes"].u8 == SENT).all() and (outs["bgr"].u8 == SENT).all(), what
        return (outs["coef"].u8.cpu().numpy().view(np.int16).reshape(n, g.mcus, g.blocks, 64),
                outs["status"].u8.cpu().numpy().view(np.int32))
    rc = L.acimg_jpeg_decode_idct(outs["coef"].ptr, quant.ptr, n, *geo, outs["planes"].ptr, sizes["planes"], st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " idct")
    rc = L.acimg_jpeg_decode_colour(outs["planes"].ptr, n, *geo, outs["bgr"].ptr, sizes["bgr"], st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " colour")
    for r, a in zip(ins, host):
        assert np.array_equal(r.u8.cpu().numpy(), a.reshape(-1).view(np.uint8)), "%s: input %s was written" % (what, r.name)
    return (outs["coef"].u8.cpu().numpy().view(np.int16).reshape(n, g.mcus, g.blocks, 64),
            outs["planes"].u8.cpu().numpy().reshape(n, -1), outs["bgr"].u8.cpu().numpy().reshape(n, g.height, g.width, 3),
            outs["status"].u8.cpu().numpy().view(np.int32))


def assert_stages(got, k, want, pillow, name):
    coef, planes, bgr, status = got
    assert status[k] == 0, "%s: status %d" % (name, status[k])
    for stage, g, w in (("coefficients", coef[k], want[0]), ("planes", planes[k], want[1]), ("pixels", bgr[k], want[2]),
                        ("pixels against Pillow", bgr[k], pillow)):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differ at %d of %d places" % (
            name, stage, int((g != w).sum()), w.size)


# ---- decode ---------------------------------------------------------------------------------------------------------------
def test_every_fixture_stream_stage_by_stage(device, golden, restated):
    for name, (data, pillow) in golden.items():
        assert_stages(device_decode(device, [data], name), 0, restated[name], pillow, name)


@pytest.mark.parametrize("H,W,full", jpeg_ref.ENCODER_SCANS)
def test_entropy_stage_returns_the_coefficients_the_encoder_was_given(device, H, W, full):
    """the oracle is the INPUT of the encoder's restatement, independent of the decoder's restatement: +-1023 in every AC
    position, DC differences of category 11, ZRL runs and blocks without an end-of-block code, three restart intervals in one
    launch.  The entropy stage alone: the IDCT of such arrays is nobody's specification."""
    files, want = jpeg_ref.encoder_files(H, W, full)
    what = "encoder scans %dx%d%s" % (W, H, ", full" if full else "")
    coef, status = device_decode(device, files, what, entropy_only=True)
    assert status.tolist() == [0, 0, 0], (what, status)
    assert coef.shape == want.shape
    bad = np.argwhere(coef != want)
    assert bad.size == 0, "%s: %d of %d coefficients differ, first at %s: %d against %d" % (
        what, len(bad), want.size, bad[0].tolist(), coef[tuple(bad[0])], want[tuple(bad[0])])
    again, status2 = device_decode(device, files, what + " (second run)", entropy_only=True)
    assert np.array_equal(again, coef) and status2.tolist() == [0, 0, 0]


def test_two_runs_of_a_batch_give_the_same_bytes(device, golden, restated):
    files = [golden[n][0] for n in FIVE]
    a, b = device_decode(device, files, "five"), device_decode(device, files, "five again")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for k, name in enumerate(FIVE):
        assert_stages(a, k, restated[name], golden[name][1], name)


@pytest.mark.parametrize("form", ("cut mid-scan", "flipped byte"))
def test_corrupt_third_image_of_five(device, golden, restated, form):
    """five images with different quant and Huffman tables and restart intervals of 0, 3, 0, 0 and 5 MCUs in one launch; the
    third is corrupt: it ends with a status, the other four are exact, nothing leaves the operands"""
    from acimg import jpeg
    files = [golden[n][0] for n in FIVE]
    good = files[2]
    info = jpeg.parse_jpeg(good)
    if form == "cut mid-scan":
        files[2] = good[:info.scan_begin + (info.scan_end - info.scan_begin) // 2]
    else:
        at = info.scan_begin + FLIP_AT
        files[2] = jref.patched(good, at, good[at] ^ 0xFF)
        assert jpeg.parse_jpeg(files[2]).scan_end == info.scan_end           # no marker was made or lost
    want_status = jref.entropy(jref.parse_stream(files[2]))[1]
    assert want_status == (jref.STATUS_EARLY_END if form == "cut mid-scan" else jref.STATUS_BAD_CODE)
    got = device_decode(device, files, form)
    print("%s: status %s, the restatement's %d" % (form, got[3].tolist(), want_status))
    assert got[3][2] != 0 and got[3][2] == want_status
    for k, name in enumerate(FIVE):
        if k != 2:
            assert_stages(got, k, restated[name], golden[name][1], name)


def test_size_queries_and_refusals(device):
    from acimg import _lib
    L = _lib.load()
    for (n, H, W, comps, hs, vs) in ((1, 1, 1, 3, 2, 2), (3, 53, 37, 3, 2, 1), (256, 256, 256, 3, 2, 2), (2, 9, 17, 1, 1, 1),
                                     (5, 65535, 40, 3, 1, 1)):
        blocks = 1 if comps == 1 else hs * vs + 2
        mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
        assert int(L.acimg_jpeg_decode_coef_bytes(n, H, W, comps, hs, vs)) == n * mcus * blocks * 64 * 2
        assert int(L.acimg_jpeg_decode_plane_bytes(n, H, W, comps, hs, vs)) == n * mcus * blocks * 64
        assert int(L.acimg_jpeg_decode_pixel_bytes(n, H, W)) == n * H * W * 3
    for bad in ((0, 8, 8, 3, 2, 2), (1, 0, 8, 3, 2, 2), (1, 8, 65536, 3, 2, 2), (1, 8, 8, 2, 1, 1), (1, 8, 8, 3, 1, 2),
                (1, 8, 8, 1, 2, 2), (1, 8, 8, 3, 4, 1)):
        assert int(L.acimg_jpeg_decode_coef_bytes(*bad)) == 0 and int(L.acimg_jpeg_decode_plane_bytes(*bad)) == 0
    assert int(L.acimg_jpeg_decode_pixel_bytes(0, 8, 8)) == 0
    buf = torch.zeros(65536, dtype=torch.uint8, device=device)
    p = buf.data_ptr()
    # refused before any launch: a null pointer, a geometry outside the scope, a buffer below its query, a misaligned slot
    assert L.acimg_jpeg_decode_entropy(None, 16, p, p, 1, p, 1, 8, 8, 3, 2, 2, p, 65536, p, None) == -1
    assert L.acimg_jpeg_decode_entropy(p, 16, p, p, 1, p, 1, 8, 8, 3, 1, 2, p, 65536, p, None) == -1
    assert "sampling 1 x 2" in _lib.last_error()
    assert L.acimg_jpeg_decode_entropy(p, 16, p, p, 1, p, 1, 8, 8, 3, 2, 2, p + 2, 65534, p, None) == -1
    assert L.acimg_jpeg_decode_entropy(p, 16, p, p, 1, p, 1, 8, 8, 3, 2, 2, p, 767, p, None) == -2
    assert L.acimg_jpeg_decode_idct(p, p, 1, 8, 8, 3, 2, 2, p, 383, None) == -2
    assert L.acimg_jpeg_decode_idct(p, None, 1, 8, 8, 3, 2, 2, p, 384, None) == -1
    assert L.acimg_jpeg_decode_colour(p, 1, 8, 8, 3, 2, 2, p, 191, None) == -2
    assert L.acimg_jpeg_decode_colour(p, 1, 8, 8, 4, 1, 1, p, 192, None) == -1
    torch.cuda.synchronize(device)
    assert not buf.any()


def test_decoder_groups_by_geometry(device, golden):
    from acimg import jpeg
    from acimg.convert import ConvertError
    names = ["noise_420_37x53", "grey_17x9", "smooth_420_37x53", "smooth_422_1x1", "restart1_420_40x72"]
    pixels, status = jpeg.JpegDecoder(device).decode([golden[n][0] for n in names], names)
    assert status.dtype == np.int32 and not status.any()
    for n, p in zip(names, pixels):
        assert p.device.type == "cuda" and p.dtype == torch.uint8 and np.array_equal(p.cpu().numpy(), golden[n][1]), n
    assert np.array_equal(jpeg.decode_jpeg(golden["q5_noise_444_17x9"][0], device), golden["q5_noise_444_17x9"][1])
    with pytest.raises(ConvertError, match="x.jpg: corrupt JPEG scan"):
        jpeg.decode_jpeg(golden["noise_420_37x53"][0][:-300], device, "x.jpg")


# ---- resampler ------------------------------------------------------------------------------------------------------------
def device_resample(device, x, rate, what):
    """the raw C ABI inside guard bands -> (fp64 [n_out], int32 [n_out]) host arrays and the filter that was used"""
    import ctypes as C

    from acimg import _lib, convert_boxes as cb, ops
    L = _lib.load()
    win, delta, num_table = cb.sinc_window(12288.0 / rate)
    formed = C.c_long(-1)
    n_out = int(L.acimg_resample_length(x.size, rate, 12288, C.byref(formed)))
    assert (formed.value, n_out) == rref.lengths(x.size, rate), what
    arena = GuardArena.for_sizes(device, [x.nbytes, win.nbytes, delta.nbytes, 8 * n_out, 4 * n_out])
    regions = []
    for a, name in ((x, "x"), (win, "win"), (delta, "delta")):
        r = arena.region(a.nbytes, name=name)
        r.u8.copy_(torch.from_numpy(a.view(np.uint8)))
        regions.append(r)
    y = arena.region(8 * n_out, fill=SENT, name="y")
    yi = arena.region(4 * n_out, fill=SENT, name="yi")
    rc = L.acimg_resample_sinc(regions[0].ptr, x.size, rate, 12288, regions[1].ptr, regions[2].ptr, win.size, num_table, y.ptr,
                               yi.ptr, n_out, ops.current_stream_handle(device))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what)
    assert L.acimg_resample_sinc(regions[0].ptr, x.size, rate, 12288, regions[1].ptr, regions[2].ptr, win.size, num_table, y.ptr,
                                 yi.ptr, n_out + 1, None) == -1
    return y.u8.cpu().numpy().view(np.float64), yi.u8.cpu().numpy().view(np.int32), (win, delta, num_table)


def assert_resampled(device, x, rate, what):
    y, yi, table = device_resample(device, x, rate, what)
    want = rref.resample_f64(x, rate, table=table)
    assert y.shape == want.shape
    bad = np.flatnonzero(y != want)
    assert bad.size == 0, "%s: %d of %d fp64 samples differ, first at %d: %r against %r" % (
        what, bad.size, y.size, bad[0], y[bad[0]], want[bad[0]])
    assert np.array_equal(yi, rref.to_int32(want)), what
    return want


@pytest.mark.parametrize("rate", RATES)
def test_resampler_equals_the_restatement(device, rate):
    rng = np.random.RandomState(rate)
    t = np.arange(3000)
    x = (rng.randn(3000) * 900 + 20000 * np.sin(2 * np.pi * 440.0 * t / rate)).astype(np.int32)
    assert_resampled(device, x, rate, "%d Hz, 3000 samples" % rate)
    assert_resampled(device, x[:50].copy(), rate, "%d Hz, 50 samples" % rate)           # every sample sees both ends
    assert_resampled(device, x[7:8].copy(), rate, "%d Hz, 1 sample" % rate)


def test_resampler_clamps_full_scale_input(device):
    """a 32-bit square wave at full scale: the filter overshoots past both ends of the int32 range"""
    x = np.where((np.arange(3000) // 5) & 1, 2 ** 31 - 1, -2 ** 31).astype(np.int32)
    for rate in (8000, 44100):
        want = assert_resampled(device, x, rate, "full scale at %d Hz" % rate)
        if rate == 8000:
            assert want.max() > 2.0 ** 31 and want.min() < -2.0 ** 31
            clamped = rref.to_int32(want)
            assert clamped.max() == 2 ** 31 - 1 and clamped.min() == -2 ** 31


def test_resampler_class(device):
    from acimg import convert_boxes as cb
    from acimg.convert import ConvertError
    rs = cb.Resampler(device)
    x = np.random.RandomState(5).randint(-2 ** 15, 2 ** 15, size=700).astype(np.int32)
    assert np.array_equal(rs.resample(x, 12288), x)                                   # passes through
    for rate in (22050, 8000):
        assert np.array_equal(rs.resample(x, rate), rref.resample(x, rate))
    with pytest.raises(ConvertError, match="one channel"):
        rs.resample(np.zeros((10, 2), np.int32), 22050, "stereo.wav")


# ---- end to end -----------------------------------------------------------------------------------------------------------
PERSONS = {"1001": [("object", 64, 4, 192, 12)],
           "1002": [("ambient sound", 10, 20, 130, 140), ("object", 0, 0, 256, 256), ("object", 33, 44, 55, 66)],
           "1003": []}
WAVS = {"1001": (22050, 16, 2500), "1002": (44100, 32, 4000), "1003": (12288, 16, 1500)}
FOLDS = {"1001": "0", "1002": "1", "1003": "1"}


@pytest.fixture(scope="module")
def tree(golden, tmp_path_factory):
    """ROOT/test_list.txt, ROOT/Dataset/Data/{0,1}/<id>.{jpg,wav}, ROOT/Dataset/Annotations/<id>.xml; the three files hold
    the 256 x 256 fixture JPEG"""
    root = tmp_path_factory.mktemp("boxes")
    raw, out = root / "raw", root / "out"
    (raw / "Dataset" / "Annotations").mkdir(parents=True)
    out.mkdir()
    jpg = golden["smooth_420_256x256"][0]
    rng = np.random.RandomState(21)
    sound = {}
    for ident, (rate, bits, n) in WAVS.items():
        d = raw / "Dataset" / "Data" / FOLDS[ident]
        d.mkdir(parents=True, exist_ok=True)
        (d / (ident + ".jpg")).write_bytes(jpg)
        amp = 2 ** (bits - 2)
        wave = rng.randn(n) * amp / 8 + amp * np.sin(2 * np.pi * 700.0 * np.arange(n) / rate)
        sound[ident] = np.clip(wave, -2 * amp, 2 * amp - 1).astype(np.int32)
        (d / (ident + ".wav")).write_bytes(convert_ref.wav_bytes(sound[ident], rate=rate, bits=bits))
        (raw / "Dataset" / "Annotations" / (ident + ".xml")).write_bytes(support.annotation_xml(ident, PERSONS[ident]))
    (raw / "test_list.txt").write_text("1002.jpg\n1001.jpg\n1003.jpg\n")
    return dict(raw=raw, out=out, sound=sound)


def test_convert_boxes_end_to_end(device, golden, tree):
    from acimg import convert_boxes as cb
    from acimg import tfio
    from acimg.data import BoxRecordLoader, box_mfcc
    raw, out = tree["raw"], tree["out"]
    assert cb.main([str(raw), str(out), "--device", str(device), "--workers", "3"]) == 0
    order = ["1001", "1002", "1003"]                                      # folder 0, then folder 1 by name
    paths = ["%s/%s.tfrecord" % (out, i) for i in order]
    assert (raw / "test.txt").read_text() == "".join(p + "\n" for p in paths)
    assert sorted(os.listdir(str(out))) == [i + ".tfrecord" for i in order]
    frame = convert_ref.resize_cubic(golden["smooth_420_256x256"][1], 224, 298)
    audio = {i: rref.resample(tree["sound"][i], WAVS[i][0]) for i in order}
    assert np.array_equal(audio["1003"], tree["sound"]["1003"])
    boxes = {"1001": [[74, 0, 0], [224, 0, 0], [4, 0, 0], [10, 0, 0]],
             "1002": [[12, 0, 38], [151, 298, 64], [18, 0, 38], [122, 224, 58]], "1003": [[0, 0, 0]] * 4}
    scene = {"1001": [1, 0, 0], "1002": [0, 1, 1], "1003": [0, 0, 0]}
    for i, p in zip(order, paths):
        with open(p, "rb") as f:
            assert f.read(2) == b"\x1f\x8b"                               # GZIP
        (rec,) = list(tfio.read_tfrecord(p))
        d = tfio.decode_box_sequence_example_native(rec)
        assert (int(d["dims"].mics), int(d["dims"].samples)) == (1, audio[i].size)
        assert np.array_equal(d["audio_samples"].reshape(-1), audio[i]), i
        assert np.array_equal(d["video_images"][0], frame), i
    (batch,) = list(BoxRecordLoader(str(raw / "test.txt"), 3))
    assert not batch[0].any() and tuple(batch[0].shape) == (3, 36, 48, 12)
    assert np.array_equal(batch[2].numpy(), np.stack([frame[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)] * 3))
    assert np.array_equal(batch[1].numpy(), np.concatenate([box_mfcc(audio[i][None]) for i in order]))
    for k in range(4):
        assert batch[3 + k].tolist() == [boxes[i][k] for i in order]
    assert batch[7].tolist() == [scene[i] for i in order]


def test_a_progressive_file_is_refused_and_nothing_of_it_is_written(device, golden, tree, tmp_path):
    from acimg import convert_boxes as cb
    from acimg.convert import ConvertError
    raw = tree["raw"]
    out = tmp_path / "out"
    out.mkdir()
    d = raw / "Dataset" / "Data" / "1"
    (d / "1004.jpg").write_bytes(jref.as_progressive(golden["smooth_420_256x256"][0]))
    (d / "1004.wav").write_bytes(convert_ref.wav_bytes(np.zeros(100), rate=12288))
    (raw / "Dataset" / "Annotations" / "1004.xml").write_bytes(support.annotation_xml("1004", []))
    listed = (raw / "test_list.txt").read_text()
    lst = str(tmp_path / "list.txt")
    try:
        (raw / "test_list.txt").write_text(listed + "1004.jpg\n")
        with pytest.raises(ConvertError, match=r"1004\.jpg: progressive JPEG"):
            cb.main([str(raw), str(out), "--device", str(device), "--list", lst])
    finally:
        (raw / "test_list.txt").write_text(listed)
        for ext in (".jpg", ".wav", ".xml"):
            os.remove(str((d if ext != ".xml" else raw / "Dataset" / "Annotations") / ("1004" + ext)))
    assert not os.path.exists(str(out / "1004.tfrecord")) and not os.path.exists(lst)
    assert os.listdir(str(out)) == []                                     # refused before a byte of its batch was written
