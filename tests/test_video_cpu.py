"""The demo clip without a GPU: the JPEG restatement (tests/jpeg_ref.py) against libjpeg and against its stored output,
the AVI writer through an independent RIFF reader (tests/avi_support.py), the PCM normalisation, the host side of the
C ABI of csrc/jpeg.hip (tables, size queries, every refusal), and the new flags of `python -m acimg.show video`.

PSNR against the source, our file and libjpeg's own file at the same quantisation tables, both decoded by libjpeg (PIL),
measured with the restatement (dB; ours, libjpeg, difference; quality / restart interval):
    smooth 224x298      50/1  41.985 41.975 +0.010    90/19 48.006 48.001 +0.006    100/7 50.909 50.643 +0.265
    overlay 224x298     50/1  26.299 26.298 +0.001    90/19 35.872 35.865 +0.008    100/7 48.818 48.719 +0.100
    noise 33x47         50/1  11.847 11.847 -0.000    90/19 12.753 12.751 +0.003    100/7 12.787 12.788 -0.001
    noise 16x16         50/1  11.905 11.905 +0.000    90/19 12.920 12.918 +0.002    100/7 12.947 12.953 -0.006
    flat 17x33          decodes exactly at every quality
The condition is ours >= libjpeg - 0.1 dB."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import avi_support  # noqa: E402
import jpeg_ref as J  # noqa: E402

GOLD = os.path.join(HERE, "golden")
SETTINGS = ((50, 1), (90, 19), (100, 7))          # quality, restart interval


def images():
    g = np.load(os.path.join(GOLD, "render_golden.npz"))
    return (("smooth", J.smooth_image()), ("overlay", J.overlay_image(g["table_gray"], g["table_jet"])),
            ("noise 33x47", J.noise_image(33, 47, 0)), ("noise 16x16", J.noise_image(16, 16, 1)),
            ("flat 17x33", np.full((17, 33, 3), 200, np.uint8)))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_against_libjpeg():
    pytest.importorskip("PIL")
    for name, img in images():
        for quality, restart in SETTINGS:
            data = J.encode(img, quality, restart)
            assert J.pil_decode(data).shape == img.shape
            ours, theirs = J.psnr_pair(img, data, quality)
            print("%-12s q %3d r %2d  ours %.3f  libjpeg %.3f  %+.3f dB  (%d bytes)" % (
                name, quality, restart, ours, theirs, ours - theirs, len(data)))
            if name.startswith("flat"):
                assert ours == float("inf") and theirs == float("inf")               # decodes exactly
            else:
                assert ours >= theirs - J.MARGIN_DB, (name, quality, restart, ours, theirs)


def test_restatement_streams_with_many_intervals_decode():
    """DRI = 1 on 33x65 gives 15 intervals: the marker index wraps; libjpeg reads every stream without a warning"""
    pytest.importorskip("PIL")
    import warnings
    img = J.noise_image(33, 65, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = J.pil_decode(J.encode(img, 90, 1))
        b = J.pil_decode(J.encode(img, 90, 5))
        c = J.pil_decode(J.encode(img, 90, 15))
    assert np.array_equal(a, b) and np.array_equal(a, c)                             # the interval does not change the picture
    assert J.encode(img, 90, 1).count(b"\xFF\xD0") == 2 and J.num_intervals(33, 65, 1) == 15    # RST0 after intervals 0 and 8


def test_restatement_reproduces_the_stored_file():
    g = np.load(os.path.join(GOLD, "jpeg_golden.npz"))
    img, quality, restart = g["image"], int(g["quality"]), int(g["restart_mcus"])
    assert img.shape == (17, 33, 3) and (quality, restart) == (90, 2)
    qt = J.quant_tables(quality)
    assert np.array_equal(qt, g["qtables"])
    coef = J.blocks(img, qt)
    assert coef.dtype == np.int16 and np.array_equal(coef, g["coef"])
    assert J.encode(img, quality, restart) == g["jfif"].tobytes()
    assert J.header(17, 33, qt, restart) + J.scan(coef, restart) + b"\xFF\xD9" == g["jfif"].tobytes()


def test_restatement_parts():
    T = J.dct_table()
    assert T[0].tolist() == [5793] * 8 and T[1].tolist() == [8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035]
    assert sorted(J.ZIGZAG.tolist()) == list(range(64)) and J.MCU_BYTES == 1245
    w = J.BitWriter()
    w.put(0xFF, 8)
    w.put(0b101, 3)
    w.pad()
    assert bytes(w.out) == b"\xFF\x00\xBF"
    # a block with one coefficient at zig-zag 63: DC 0, three ZRL, then run 14 / size 1
    zz = np.zeros(64, np.int16)
    zz[63] = 1
    w = J.BitWriter()
    J.encode_block(w, zz, 0, 0)
    bits = [J.DC_TABLES[0][0], J.AC_TABLES[0][0xF0], J.AC_TABLES[0][0xF0], J.AC_TABLES[0][0xF0], J.AC_TABLES[0][0xE1], (1, 1)]
    v = J.BitWriter()
    for code, length in bits:
        v.put(code, length)
    assert (bytes(w.out), w.acc, w.n) == (bytes(v.out), v.acc, v.n)
    assert J._magnitude(-1023) == (10, 0) and J._magnitude(1016 + 1024) == (11, 2040) and J._magnitude(-3) == (2, 0)


def test_package_header_equals_the_restatement():
    """acimg/jpeg.py builds the header segments from its own copy of the tables"""
    from acimg import jpeg
    for H, W, q, r in ((17, 33, 90, 2), (224, 298, 50, 19), (1, 65535, 100, 65535)):
        assert jpeg.jfif_header(H, W, J.quant_tables(q), r) == J.header(H, W, J.quant_tables(q), r)
    assert tuple(J.ZIGZAG.tolist()) == jpeg.ZIGZAG


# ---- AVI ---------------------------------------------------------------------------------------------------------------
def test_avi_round_trip(tmp_path):
    from acimg.avi import AviWriter
    rng = np.random.RandomState(5)
    frames = [bytes(rng.randint(0, 256, size=n).astype(np.uint8)) for n in (101, 64, 1, 250, 77)]     # odd and even
    pcm = rng.randint(-32768, 32768, size=(5, 1024)).astype(np.int16)
    path = str(tmp_path / "clip.avi")
    w = AviWriter(path, 298, 224, 12, 12288)
    for f, p in zip(frames, pcm):
        w.add_frame(f, p)
    size = w.close()
    assert w.close() == size                                                          # closing twice is harmless
    with open(path, "rb") as f:
        buf = f.read()
    assert size == len(buf) == os.path.getsize(path)
    avi = avi_support.parse(buf)
    assert avi["order"] == [b"hdrl", b"movi", b"idx1"]
    h = avi["avih"]
    assert h["dwTotalFrames"] == 5 and h["dwStreams"] == 2 and (h["dwWidth"], h["dwHeight"]) == (298, 224)
    assert h["dwMicroSecPerFrame"] == 1000000 // 12 and h["dwFlags"] == 0x110
    assert h["dwSuggestedBufferSize"] == 2048
    v, a = avi["streams"]
    assert (v["strh"]["fccType"], v["strh"]["fccHandler"]) == (b"vids", b"MJPG")
    assert (v["strh"]["dwScale"], v["strh"]["dwRate"], v["strh"]["dwLength"]) == (1, 12, 5)
    assert (v["strh"]["right"], v["strh"]["bottom"]) == (298, 224) and v["strh"]["dwSuggestedBufferSize"] == 250
    bi = avi_support.bitmap_info(v["strf"])
    assert len(v["strf"]) == 40 and bi == dict(biSize=40, biWidth=298, biHeight=224, biPlanes=1, biBitCount=24,
                                               biCompression=b"MJPG", biSizeImage=298 * 224 * 3)
    assert a["strh"]["fccType"] == b"auds" and a["strh"]["dwSampleSize"] == 2
    assert (a["strh"]["dwScale"], a["strh"]["dwRate"], a["strh"]["dwLength"]) == (1, 12288, 5 * 1024)
    assert avi_support.wave_format(a["strf"]) == dict(wFormatTag=1, nChannels=1, nSamplesPerSec=12288,
                                                      nAvgBytesPerSec=24576, nBlockAlign=2, wBitsPerSample=16, cbSize=0)
    ch = avi["chunks"]
    assert [c["fourcc"] for c in ch] == [b"00dc", b"01wb"] * 5                         # picture, then its sound
    for i in range(5):
        assert ch[2 * i]["data"] == frames[i] and ch[2 * i + 1]["data"] == pcm[i].astype("<i2").tobytes()
        assert ch[2 * i]["pad"] == (b"\x00" if len(frames[i]) & 1 else None)          # the pad byte of an odd payload
        assert ch[2 * i]["offset"] % 2 == 0 and ch[2 * i + 1]["offset"] % 2 == 0
    assert ch[0]["offset"] == 4                                                        # right behind the 'movi' fourcc
    idx = avi["index"]
    assert len(idx) == 10 and all(e["flags"] == 0x10 for e in idx)                     # every chunk a key frame
    for e, c in zip(idx, ch):
        assert (e["fourcc"], e["offset"], e["size"]) == (c["fourcc"], c["offset"], c["size"])
        at = avi["movi"] + e["offset"]                                                 # offsets count from the 'movi' fourcc
        assert buf[at:at + 4] == e["fourcc"] and struct.unpack_from("<I", buf, at + 4)[0] == e["size"]


def test_avi_refusals_and_bytes_input(tmp_path):
    from acimg.avi import AviWriter
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / "a.avi"), 0, 224, 12, 12288)
    with AviWriter(str(tmp_path / "b.avi"), 16, 16, 12, 12288) as w:
        w.add_frame(b"\xFF\xD8\xFF\xD9", b"\x01\x00\x02\x00")
        with pytest.raises(ValueError):
            w.add_frame(b"x", b"\x01\x00\x02")                                         # half a sample
    with pytest.raises(ValueError):
        w.add_frame(b"x", b"")                                                         # closed
    with open(str(tmp_path / "b.avi"), "rb") as f:
        avi = avi_support.parse(f.read())
    assert avi["avih"]["dwTotalFrames"] == 1 and avi["streams"][1]["strh"]["dwLength"] == 2
    assert avi["chunks"][1]["data"] == b"\x01\x00\x02\x00"


def test_pcm_normalisation():
    from acimg.avi import normalize_pcm
    assert normalize_pcm(np.zeros((3, 1024), np.int32)).tolist() == [0] * 3072         # a silent clip stays zeros
    assert normalize_pcm(np.zeros(0, np.int32)).shape == (0,)
    x = np.array([[0, 100, -400], [200, 399, -1]], np.int32)                           # the peak is a negative sample
    got = normalize_pcm(x)
    want = np.rint(x.reshape(-1).astype(np.float64) / 400.0 * 32767.0).astype(np.int16)
    assert got.dtype == np.int16 and got.tolist() == want.tolist() == [0, 8192, -32767, 16384, 32685, -82]
    edge = normalize_pcm(np.array([-2147483648, 2147483647, 1], np.int32))             # |int32 min| does not overflow
    assert edge.tolist() == [-32767, 32767, 0]


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


def test_quant_tables_follow_the_formula(lib):
    from acimg import _lib, jpeg
    for q in (1, 49, 50, 100):
        out = np.zeros(128, np.uint8)
        assert lib.acimg_jpeg_quant_tables(q, out.ctypes.data_as(C.c_void_p)) == 0
        s = 5000 // q if q < 50 else 200 - 2 * q
        want = np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (J.LUMA_Q, J.CHROMA_Q)])
        assert np.array_equal(out.reshape(2, 64), want), q
        assert np.array_equal(jpeg.quant_tables(q), want)
    assert (J.quant_tables(100) == 1).all() and (J.quant_tables(1) == 255).all()
    assert J.quant_tables(50)[0].tolist() == J.LUMA_Q.tolist()
    out = np.zeros(128, np.uint8)
    for q in (0, 101, -5):
        assert lib.acimg_jpeg_quant_tables(q, out.ctypes.data_as(C.c_void_p)) == -1 and "quality" in _lib.last_error()
    assert lib.acimg_jpeg_quant_tables(90, None) == -1
    with pytest.raises(_lib.AcimgError):
        jpeg.quant_tables(0)


def test_size_queries_follow_their_formulas(lib):
    for n, H, W, r in ((1, 16, 16, 1), (2, 17, 33, 2), (12, 224, 298, 19), (1, 32, 144, 7), (3, 65535, 1, 65535)):
        mh, mw = -(-H // 16), -(-W // 16)
        mcus = mh * mw
        intervals = -(-mcus // r)
        assert lib.acimg_jpeg_coef_bytes(n, H, W) == n * mcus * 6 * 64 * 2
        assert lib.acimg_jpeg_scan_capacity(H, W, r) == 2490 * mcus + 4 * intervals == J.scan_capacity(H, W, r)
        lens, bits = -(-(n * intervals * 8) // 16) * 16, -(-(n * mcus * 4) // 16) * 16
        assert lib.acimg_jpeg_scan_workspace(n, H, W, r) == lens + bits + n * mcus * 1248 + n * intervals * (2490 * r + 2)
    assert lib.acimg_jpeg_scan_capacity(224, 298, 19) == 2490 * 266 + 4 * 14
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 65536)):
        assert lib.acimg_jpeg_coef_bytes(*bad) == 0
    for bad in ((0, 16, 1), (16, 65536, 1), (16, 16, 0), (16, 16, 65536)):
        assert lib.acimg_jpeg_scan_capacity(*bad) == 0 and lib.acimg_jpeg_scan_workspace(1, *bad) == 0
    assert lib.acimg_jpeg_scan_workspace(0, 16, 16, 1) == 0


def test_refusals_precede_any_launch(lib):
    """every argument but the refused one is plausible; the pointers are never followed, because nothing is launched"""
    from acimg import _lib
    P = 0x10000                                                                        # 16-byte aligned, not null
    cap = lib.acimg_jpeg_scan_capacity(17, 33, 2)
    ws = lib.acimg_jpeg_scan_workspace(2, 17, 33, 2)

    def blocks(rgb=P, n=2, H=17, W=33, qt=P, coef=P):
        return lib.acimg_jpeg_blocks(rgb, n, H, W, qt, coef, None)

    def scan(coef=P, n=2, H=17, W=33, r=2, out=P, stride=cap, nbytes=P, w=P, wb=ws):
        return lib.acimg_jpeg_scan(coef, n, H, W, r, out, stride, nbytes, w, wb, None)

    for kw in (dict(rgb=None), dict(qt=None), dict(coef=None), dict(n=0), dict(n=65536), dict(H=0), dict(H=65536), dict(W=0),
               dict(W=65536)):
        assert blocks(**kw) == -1, kw
    for kw, word in ((dict(coef=None), "null"), (dict(out=None), "null"), (dict(nbytes=None), "null"), (dict(w=None), "null"),
                     (dict(n=0), "positive"), (dict(H=0), "outside"), (dict(H=65536), "outside"), (dict(W=0), "outside"),
                     (dict(W=65536), "outside"), (dict(r=0), "restart_mcus"), (dict(r=65536), "restart_mcus"),
                     (dict(stride=cap - 1), "frame_stride"), (dict(coef=P + 2), "aligned"), (dict(w=P + 4), "aligned")):
        assert scan(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert scan(wb=ws - 1) == -2 and "workspace" in _lib.last_error()
    # a frame whose capacity does not fit the int32 of scan_bytes
    big = lib.acimg_jpeg_scan_capacity(65535, 65535, 65535)
    assert big > 2 ** 31 and lib.acimg_jpeg_scan(P, 1, 65535, 65535, 65535, P, big, P, P, 2 ** 62, None) == -1
    assert "int32" in _lib.last_error()


def test_signatures_and_version(lib):
    from acimg import _lib
    I, P, SZ = C.c_int, C.c_void_p, C.c_size_t
    assert _lib.PROTOTYPES["acimg_jpeg_quant_tables"] == (I, [I, P])
    assert _lib.PROTOTYPES["acimg_jpeg_coef_bytes"] == (SZ, [I, I, I])
    assert _lib.PROTOTYPES["acimg_jpeg_blocks"] == (I, [P, I, I, I, P, P, P])
    assert _lib.PROTOTYPES["acimg_jpeg_scan_capacity"] == (SZ, [I, I, I])
    assert _lib.PROTOTYPES["acimg_jpeg_scan_workspace"] == (SZ, [I, I, I, I])
    assert _lib.PROTOTYPES["acimg_jpeg_scan"] == (I, [P, I, I, I, I, P, SZ, P, P, SZ, P])
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "acimg.h")).read()
    for name in ("acimg_jpeg_quant_tables", "acimg_jpeg_coef_bytes", "acimg_jpeg_blocks", "acimg_jpeg_scan_capacity",
                 "acimg_jpeg_scan_workspace", "acimg_jpeg_scan"):
        assert name + "(" in hdr and lib[name] is not None
    assert lib.acimg_version() == 207                                                  # the entries were added without a bump


# ---- the command line ------------------------------------------------------------------------------------------------
BASE = ["--train_file", "/data/class_1/video_4/testing.txt", "--init_checkpoint", "/ck/epoch_7.ckpt"]


def test_show_video_flags():
    from acimg import show
    a = show.parse_args(["video"] + BASE)
    assert (a.avi, a.quality, a.restart_mcus) == (0, 90, None)
    a = show.parse_args(["video"] + BASE + ["--avi", "1", "--quality", "75", "--restart_mcus", "4"])
    assert (a.avi, a.quality, a.restart_mcus) == (1, 75, 4)
    assert show.avi_file(a) == "/data/class_1/video_4/video_boat_video_4_7.avi"
    assert show.ffmpeg_commands(a)[1].endswith(" " + show.avi_file(a))                 # the merge command's target
    assert not show.avi_file(a).startswith(show.output_dir(a))
    assert show.SAMPLE_RATE == 12288 and show.FPS == 12
    for cmd in ("images", "boxes"):
        for flag in (["--avi", "1"], ["--quality", "90"], ["--restart_mcus", "1"]):
            with pytest.raises(SystemExit):
                show.parse_args([cmd] + BASE + flag)
    with pytest.raises(SystemExit):
        show.parse_args(["video"] + BASE + ["--avi", "2"])


def test_summary_without_avi_keeps_its_keys(tmp_path):
    from acimg import show
    train = str(tmp_path / "class_1" / "video_4" / "testing.txt")
    a = show.parse_args(["video", "--train_file", train, "--init_checkpoint", "/ck/epoch_7.ckpt"])
    os.makedirs(show.output_dir(a))
    res = show.write_summary(a, 24, 298)
    old = ["command", "num_frames", "file_pattern", "directory", "height", "width", "checkpoint", "fps", "printf_pattern",
           "ffmpeg"]
    assert list(res) == old
    with open(os.path.join(show.output_dir(a), "show.json")) as f:
        assert list(json.load(f)) == old
    more = show.write_summary(a, 24, 298, extra=dict(avi="x.avi", avi_bytes=7, quality=90, restart_mcus=19, sample_rate=12288))
    assert list(more) == old + ["avi", "avi_bytes", "quality", "restart_mcus", "sample_rate"]
    assert {k: more[k] for k in old} == res


def test_loader_signature_keeps_its_default():
    import inspect

    from acimg.data import TFRecordDataLoader
    p = inspect.signature(TFRecordDataLoader.__init__).parameters
    assert p["raw_audio"].default is False and list(p)[-1] == "raw_audio"
