"""The device checksums and the record gather (csrc/checksum.hip) on the GPU.  Every operand of both entry points lies inside
guard bands (tests/guard_arena.py).  The oracles are zlib.crc32, zlib.adler32 and the library's host acimg_crc32c: every
value is compared bit for bit, nothing has a tolerance.  Then the consumers: `gzip_many` / `zlib_many`, the converter with
`--assemble device` against `--assemble host` file for file, `png.encode_png_many` and the device branch of
`python -m acimg.show` against `encode_png`."""
import gzip
import os
import struct
import sys
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import checksum_ref as ref  # noqa: E402
import convert_ref  # noqa: E402
from data_support import outdoor_record  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B
KINDS = (0, 1, 2, 3)
KIND_IDS = ["crc32", "crc32c", "crc32c_masked", "adler32"]


@pytest.fixture(scope="module")
def packed_set():
    """the payloads of checksum_ref.payload_set and, per kind, the oracles' values; computed once, shared, never modified"""
    payloads = ref.payload_set()
    return payloads, {kind: [ref.oracle(kind, p) for _, p in payloads] for kind in KINDS}


def guarded_checksum(device, payloads, kind, what, shift=0, store=None):
    """one acimg_checksum call on `payloads`, packed back to back `shift` bytes into their region, with input, output,
    workspace and the store target inside guard bands -> (values, the store region's bytes or None)"""
    from acimg import _lib, ops
    L = _lib.load()
    lengths = [len(p) for p in payloads]
    total, count = sum(lengths), len(payloads)
    ws_bytes = L.acimg_checksum_workspace(total, count)
    assert ws_bytes > 0
    sizes = [total + shift + 1, 4 * count, ws_bytes] + ([store[0]] if store else [])
    arena = GuardArena.for_sizes(device, sizes)
    src = arena.region(total + shift + 1, fill=0xEE, name="in")
    out = arena.region(4 * count, fill=SENT, name="out")
    ws = arena.region(ws_bytes, fill=SENT, name="ws")
    target = arena.region(store[0], fill=SENT, name="store") if store else None
    if total:
        src.u8[shift:shift + total].copy_(torch.from_numpy(np.frombuffer(b"".join(payloads), np.uint8).copy()))
    _lib.check(L.acimg_checksum(src.ptr + shift, ref.longs(*lengths), count, kind, out.ptr, target.ptr if store else None,
                                ref.longs(*store[1]) if store else None, ws.ptr, ws_bytes, ops.current_stream_handle(device)), what)
    torch.cuda.synchronize(device)
    arena.check(what)
    values = [int(v) for v in out.view(torch.int32, count).cpu().numpy().view(np.uint32)]
    return values, (target.u8.cpu().numpy().tobytes() if store else None)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_every_length_in_one_packed_call(device, packed_set, kind):
    """all payloads in ONE call, one behind the other from an odd address: every start is unaligned; a second run gives the
    same bits"""
    payloads, want = packed_set
    got, _ = guarded_checksum(device, [p for _, p in payloads], kind, KIND_IDS[kind], shift=3)
    bad = [(name, hex(g), hex(w)) for (name, _), g, w in zip(payloads, got, want[kind]) if g != w]
    assert not bad, "%d of %d payloads differ from the oracle: %s" % (len(bad), len(got), bad[:6])
    again, _ = guarded_checksum(device, [p for _, p in payloads], kind, KIND_IDS[kind] + " (second run)", shift=3)
    assert again == got
    assert want[kind][[n for n, _ in payloads].index("known")] == {0: 0xCBF43926, 1: 0xE3069283, 2: ref.mask(0xE3069283),
                                                                   3: 0x091E01DE}[kind]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_one_payload_and_the_empty_one(device, kind):
    rng = np.random.RandomState(41)
    data = rng.randint(0, 256, 1000).astype(np.uint8).tobytes()
    for shift in (0, 1, 15):
        assert guarded_checksum(device, [data], kind, "count = 1", shift=shift)[0] == [ref.oracle(kind, data)]
    assert guarded_checksum(device, [b""], kind, "one empty payload")[0] == [ref.oracle(kind, b"")]
    assert guarded_checksum(device, [b"", b"", b"\x00", b""], kind, "empty payloads")[0] == \
        [ref.oracle(kind, b"")] * 2 + [ref.oracle(kind, b"\x00"), ref.oracle(kind, b"")]
    assert [ref.oracle(k, b"") for k in KINDS] == [0, 0, 0xa282ead8, 1]


@pytest.mark.parametrize("kind", (2, 0), ids=["crc32c_masked", "crc32"])
def test_store_at_every_byte_alignment(device, kind):
    rng = np.random.RandomState(42)
    payloads = [rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in (100, 0, 7, 20000, 33)]
    at = [64, 69, -1, 74, 79]                                             # 0, 1, 2, 3 mod 4, and one payload without a store
    values, stored = guarded_checksum(device, payloads, kind, "store_at", shift=5, store=(128, at))
    assert values == [ref.oracle(kind, p) for p in payloads]
    want = bytearray([SENT]) * 128
    for v, o in zip(values, at):
        if o >= 0:
            want[o:o + 4] = struct.pack("<I", v)
    assert stored == bytes(want)


def test_device_checksum_class(device):
    from acimg.checksum import ADLER32, CRC32, CRC32C, CRC32C_MASKED, DeviceChecksum
    rng = np.random.RandomState(43)
    dc = DeviceChecksum(device)
    a, b = rng.randint(0, 256, 70001).astype(np.uint8), rng.randint(0, 256, 19).astype(np.uint8)
    mixed = [a.tobytes(), torch.from_numpy(b).to(device), b"", torch.from_numpy(a[:5].copy()), bytearray(b"123456789")]
    as_bytes = [a.tobytes(), b.tobytes(), b"", a[:5].tobytes(), b"123456789"]
    for kind in (CRC32, CRC32C, CRC32C_MASKED, ADLER32):
        assert dc.many(mixed, kind) == [ref.oracle(kind, p) for p in as_bytes]
    assert dc.many([], CRC32) == [] and dc.many([b""], ADLER32) == [1]
    assert dc.crc32(ref.KNOWN) == 0xCBF43926 and dc.crc32c(ref.KNOWN) == 0xE3069283 and dc.adler32(ref.KNOWN) == 0x091E01DE
    assert dc.crc32c(ref.KNOWN, masked=True) == ref.mask(0xE3069283)
    base = torch.full((32,), SENT, dtype=torch.uint8, device=device)
    got = dc.many([a.tobytes(), b.tobytes()], CRC32, store=(base, [-1, 9]))
    assert base.cpu().numpy().tobytes() == bytes([SENT]) * 9 + struct.pack("<I", got[1]) + bytes([SENT]) * 19
    with pytest.raises(ValueError):
        dc.many([b"abc"], CRC32, store=(base, [30]))


# ---- the gather ------------------------------------------------------------------------------------------------------------
def test_record_gather_is_a_byte_exact_copy(device):
    from acimg import _lib, ops
    L = _lib.load()
    rng = np.random.RandomState(44)
    big = 9 * 16384 + 5                                                   # more than one pass of the grid's eight chunk rows
    src = [rng.randint(0, 256, 160 * 1024).astype(np.uint8) for _ in range(2)]
    dst_bytes = 32768 + 4 + big + 100
    rows, at = [], 7
    # abutting segments from both sources; 4097 bytes congruent mod 4 only, the others at odd offsets
    for i, n in enumerate((0, 1, 3, 4, 5, 15, 16, 17, 4097)):
        rows.append((at, at + 4 if n == 4097 else 1000 + 37 * i, n, i & 1))
        at += n
    assert at < 8192
    for dm in range(16):                                                  # every dst_off mod 16 against every src_off mod 16
        for sm in range(16):
            k = dm * 16 + sm
            rows.append((8192 + 64 * k + dm, 20000 + 48 * k + sm, 33, (dm + sm) & 1))
    rows.append((32768 + 4, 20, big, 1))                                  # congruent mod 16: head, 16-byte body, tail
    rows.append((dst_bytes - 50, 77, 0, 0))
    nseg = len(rows)
    ws_bytes = L.acimg_record_gather_workspace(nseg)
    arena = GuardArena.for_sizes(device, [src[0].size, src[1].size, dst_bytes, ws_bytes])
    s0, s1 = arena.region(src[0].size, name="src0"), arena.region(src[1].size, name="src1")
    dst = arena.region(dst_bytes, fill=SENT, name="dst")
    ws = arena.region(ws_bytes, fill=SENT, name="ws")
    s0.u8.copy_(torch.from_numpy(src[0]))
    s1.u8.copy_(torch.from_numpy(src[1]))
    want = np.full(dst_bytes, SENT, np.uint8)
    for d, s, n, which in rows:
        want[d:d + n] = src[which][s:s + n]
    for run in range(2):
        _lib.check(L.acimg_record_gather(s0.ptr, s1.ptr, ref.longs(*[v for r in rows for v in r]), nseg, dst.ptr, dst_bytes, ws.ptr,
                                         ws_bytes, ops.current_stream_handle(device)), "record_gather")
        torch.cuda.synchronize(device)
        arena.check("record_gather")
        got = dst.u8.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "run %d: %d bytes differ, first at %d (got %d, want %d)" % (run, bad.size, bad[0], got[bad[0]],
                                                                                          want[bad[0]])
    assert np.array_equal(s0.u8.cpu().numpy(), src[0]) and np.array_equal(s1.u8.cpu().numpy(), src[1])
    # one source alone; the other may be null
    dst.fill(SENT)
    _lib.check(L.acimg_record_gather(None, s1.ptr, ref.longs(5, 3, 40, 1), 1, dst.ptr, dst_bytes, ws.ptr, ws_bytes,
                                     ops.current_stream_handle(device)), "record_gather")
    torch.cuda.synchronize(device)
    arena.check("record_gather, src1 alone")
    got = dst.u8[:64].cpu().numpy()
    assert (got[:5] == SENT).all() and np.array_equal(got[5:45], src[1][3:43]) and (got[45:] == SENT).all()


# ---- containers ------------------------------------------------------------------------------------------------------------
def test_containers_of_device_tensors_equal_the_host_form(device):
    from acimg.deflate import DeviceDeflater
    rng = np.random.RandomState(45)
    dd = DeviceDeflater(device)
    smooth = ((np.arange(50000) // 7) % 251).astype(np.uint8).tobytes()
    payloads = [smooth, b"", rng.randint(0, 256, 16385).astype(np.uint8).tobytes(), b"abcde", b"\xff" * 5553]
    on_device = [torch.from_numpy(np.frombuffer(p, np.uint8).copy()).to(device) for p in payloads]
    mixed = [on_device[0], payloads[1], payloads[2], on_device[3], on_device[4]]
    want_gzip, want_zlib = [dd.gzip(p) for p in payloads], [dd.zlib(p) for p in payloads]
    for form in (on_device, payloads, mixed):
        assert dd.gzip_many(form) == want_gzip
        assert dd.zlib_many(form) == want_zlib
    for p, g, z in zip(payloads, want_gzip, want_zlib):
        assert gzip.decompress(g) == p and zlib.decompress(z) == p
    assert dd.gzip_many([]) == [] and dd.zlib_many([on_device[1]]) == [dd.zlib(b"")]
    assert dd.compress_many(mixed) == [dd.deflate(p) for p in payloads]


# ---- the converter ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_tree(tmp_path_factory):
    """a two-second recording at the smallest accepted frame size, 224 x 298 (written once, never modified)"""
    rng = np.random.RandomState(46)
    raw = tmp_path_factory.mktemp("assemble") / "raw"
    raw.mkdir()
    ramp = (np.arange(224)[:, None, None] + np.arange(298)[None, :, None] // 2 + np.arange(3)[None, None, :] * 9) % 256
    frames = (ramp[None] + rng.randint(0, 3, size=(24, 224, 298, 3))).astype(np.uint8)
    sound = rng.randint(-2 ** 15, 2 ** 15, size=2 * 12288 + 5)
    convert_ref.write_recording(raw, 2, 4, 2, frames, sound)
    return str(raw)


@pytest.mark.parametrize("modalities", [None, (1,), (2,)], ids=["all", "audio", "video"])
def test_assemble_device_writes_the_files_of_assemble_host(device, raw_tree, tmp_path, modalities):
    from acimg import convert, tfio
    from acimg.data import TFRecordDataLoader
    files = {}
    for mode in ("host", "device"):
        out = tmp_path / mode
        out.mkdir()
        lst = str(out / "list.txt")
        argv = [raw_tree, str(out), "--list", lst, "--device", str(device), "--workers", "2", "--deflate", "device",
                "--assemble", mode]
        if modalities is not None:
            argv += ["--modalities"] + [str(m) for m in modalities]
        assert convert.main(argv) == 0
        paths = open(lst).read().split()
        assert len(paths) == 2
        files[mode] = (lst, paths, [open(p, "rb").read() for p in paths])
    assert [os.path.relpath(p, str(tmp_path / "host")) for p in files["host"][1]] == \
        [os.path.relpath(p, str(tmp_path / "device")) for p in files["device"][1]]
    for k, (a, b) in enumerate(zip(files["host"][2], files["device"][2])):
        assert a == b, "record %d: --assemble device wrote %d bytes, --assemble host %d" % (k + 1, len(b), len(a))
    lst, paths, _ = files["device"]
    want_lists = [k for k, m in (("audio/data", 1), ("video/image", 2)) if modalities is None or m in modalities]
    for p in paths:
        (rec,) = list(tfio.read_tfrecord(p, "GZIP", verify=True))
        ctx, lists = tfio.parse_sequence_example(rec)
        assert list(lists) == want_lists and all(len(v) == 12 for v in lists.values())
        assert int(ctx["classes"][0]) == 2 and int(ctx["location"][0]) == 4
    if modalities is None:                                                 # the loader reads records with audio and video
        batches = list(TFRecordDataLoader(lst, 12, device=device, modalities=(1, 2)).data)
        assert len(batches) == 2 and all(tuple(b[2].shape) == (12, 224, 298, 3) for b in batches)


def test_converter_keyword_and_times(device, raw_tree, tmp_path):
    from acimg import convert
    paths, conv = convert.convert(raw_tree, str(tmp_path), device=str(device), workers=1, deflate="device", assemble="device")
    assert len(paths) == 2 and sorted(conv.times) == ["deflate", "device", "read"] and all(v > 0 for v in conv.times.values())
    assert sorted(conv._assembler.free) == list(range(6))                  # every slot is free again


# ---- PNG -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 5, 7), (2, 224, 298)])
def test_encode_png_many_equals_encode_png(device, n, h, w):
    from acimg import png
    from acimg.deflate import DeviceDeflater
    rng = np.random.RandomState(47)
    img = ((np.arange(h)[:, None, None] + np.arange(w)[None, :, None] // 2 + np.arange(3) * 40)[None] % 256
           + rng.randint(0, 2, (n, h, w, 3))).astype(np.uint8)
    dd = DeviceDeflater(device)
    want = [png.encode_png(f, deflater=dd) for f in img]
    assert png.encode_png_many(torch.from_numpy(img).to(device), dd) == want
    assert png.encode_png_many(img, dd) == want
    assert png.encode_png_many(img[:0], dd) == []
    with pytest.raises(ValueError):
        png.encode_png_many(img[0], dd)


def test_show_device_branch_writes_encode_png_of_the_same_pixels(device, tmp_path, monkeypatch):
    from acimg import png, show, tfio
    from acimg.deflate import DeviceDeflater
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    from render_ref import read_png

    rng = np.random.RandomState(48)
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    tr._build_functions(batch_size=3)
    tr.modelimages.initialize()
    tr.modelac.initialize()
    ckdir = tmp_path / "ckpt"
    ckdir.mkdir()
    ckpt = str(ckdir / "epoch_7.ckpt")
    tfio.write_checkpoint(ckpt, OrderedDict((k, v.numpy()) for k, v in tr.session.store.state_dict().items()))
    vdir = tmp_path / "class_1" / "video_4"
    vdir.mkdir(parents=True)
    tfio.write_tfrecord(str(vdir / "o0.tfrecord"), [outdoor_record(rng, 2, 7, wide=False)], compression="GZIP")
    (vdir / "testing.txt").write_text(str(vdir / "o0.tfrecord") + "\n")
    common = ["video", "--train_file", str(vdir / "testing.txt"), "--init_checkpoint", ckpt, "--batch_size", "3",
              "--num_skip_conn", "1", "--ae", "0"]
    args = show.parse_args(common + ["--png_deflate", "device"])
    seen = []                                                              # the pixels the device branch hands to the encoder

    def recording(frames, deflater):
        seen.extend(frames.cpu().numpy())
        return png_many(frames, deflater)
    png_many = png.encode_png_many
    monkeypatch.setattr(png, "encode_png_many", recording)
    res = show.run(args, trainer=show.build_trainer(args, device), log=lambda *a: None)
    d = show.output_dir(args)
    names = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    assert res["num_frames"] == 12 and len(names) == 12 and len(seen) == 12
    dd = DeviceDeflater(device)
    for name, pixels in zip(names, seen):
        data = open(os.path.join(d, name), "rb").read()
        assert pixels.shape == (224, 298, 3) and np.array_equal(read_png(data), pixels), name
        assert data == png.encode_png(pixels, deflater=dd), name           # what write_png(..., deflater=) wrote before
