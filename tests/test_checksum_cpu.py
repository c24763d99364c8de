"""The checksum feature without a GPU: the algebra of tests/checksum_ref.py against zlib and acimg_crc32c, the record
layout builder of acimg/tfio.py against `frame_record(build_record(...))`, the host-side refusals of `acimg_checksum` and
`acimg_record_gather` (fake pointers: a call that is not refused reaches a launch and comes back as ACIMG_ELAUNCH), and the
converter's `--assemble` switch."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import checksum_ref as ref

EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


def crc32c_host(lib, data):
    data = bytes(data)
    return int(lib.acimg_crc32c(data, len(data), 0))


# ---- the algebra -----------------------------------------------------------------------------------------------------------
def test_known_vector(lib):
    assert ref.crc(ref.KNOWN, ref.POLY["crc32"]) == zlib.crc32(ref.KNOWN) == ref.KNOWN_VALUES["crc32"] == 0xCBF43926
    assert ref.crc(ref.KNOWN, ref.POLY["crc32c"]) == crc32c_host(lib, ref.KNOWN) == ref.KNOWN_VALUES["crc32c"] == 0xE3069283
    assert ref.adler_in_pieces(ref.KNOWN, [4]) == zlib.adler32(ref.KNOWN) == ref.KNOWN_VALUES["adler32"] == 0x091E01DE


@pytest.mark.parametrize("name", sorted(ref.POLY))
def test_field_arithmetic(name):
    poly = ref.POLY[name]
    rng = np.random.RandomState(3)
    assert ref.mulx(ref.xinv(poly), poly) == ref.ONE and ref.gf_mul(ref.xinv(poly), ref.X, poly) == ref.ONE
    assert ref.xpow(0, poly) == ref.ONE and ref.xpow(1, poly) == ref.X and ref.xpow(32, poly) == poly
    v = ref.ONE
    for e in range(1, 70):
        v = ref.mulx(v, poly)
        assert ref.xpow(e, poly) == v
    for _ in range(20):
        a, b, c = (int(x) for x in rng.randint(0, 2 ** 32, 3, dtype=np.uint64))
        assert ref.gf_mul(a, b, poly) == ref.gf_mul(b, a, poly)
        assert ref.gf_mul(a, ref.ONE, poly) == a
        assert ref.gf_mul(a, b ^ c, poly) == ref.gf_mul(a, b, poly) ^ ref.gf_mul(a, c, poly)
        assert ref.gf_mul(ref.gf_mul(a, b, poly), c, poly) == ref.gf_mul(a, ref.gf_mul(b, c, poly), poly)
    e1, e2 = 8 * 123457, 8 * 16384
    assert ref.gf_mul(ref.xpow(e1, poly), ref.xpow(e2, poly), poly) == ref.xpow(e1 + e2, poly)
    assert ref.gf_mul(ref.xpow(e1, poly), ref.gf_pow(ref.xinv(poly), e1, poly), poly) == ref.ONE


def test_pieces_against_the_oracles(lib):
    rng = np.random.RandomState(11)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 1000, 5553, 40000):
        data = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        for fill in (data, bytes(n), b"\xff" * n):
            cuts = sorted(int(c) for c in rng.randint(0, n + 1, 4))
            assert ref.crc_in_pieces(fill, cuts, ref.POLY["crc32"]) == zlib.crc32(fill), (n, cuts)
            assert ref.crc_in_pieces(fill, cuts, ref.POLY["crc32c"]) == crc32c_host(lib, fill), (n, cuts)
            assert ref.adler_in_pieces(fill, cuts) == zlib.adler32(fill), (n, cuts)
    # leading zeros are free, trailing zeros multiply by x^8 each: what the window plan rests on
    poly = ref.POLY["crc32"]
    d = rng.randint(0, 256, 77).astype(np.uint8).tobytes()
    assert ref.pure(bytes(9) + d, poly) == ref.pure(d, poly)
    assert ref.pure(d + bytes(9), poly) == ref.gf_mul(ref.pure(d, poly), ref.xpow(72, poly), poly)
    assert ref.finish(ref.pure(d, poly), len(d), poly) == zlib.crc32(d)
    assert ref.mask(0) == ref.MASK_DELTA


def test_the_window_plan(lib):
    rng = np.random.RandomState(12)
    window = rng.randint(0, 256, ref.SEGMENT).astype(np.uint8).tobytes()
    for name, poly in ref.POLY.items():
        assert ref.window_by_lanes(window, poly) == ref.pure(window, poly), name
    for n, address in ((0, 5), (1, 16383), (2, 16383), (70, 1), (ref.SEGMENT, 0), (ref.SEGMENT, 7), (2 * ref.SEGMENT + 3, 16381),
                       (40000, 123457)):
        data = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        assert ref.crc_by_windows(data, address, ref.POLY["crc32"]) == zlib.crc32(data), (n, address)
        assert ref.crc_by_windows(data, address, ref.POLY["crc32c"]) == crc32c_host(lib, data), (n, address)
    assert ref.crc_by_windows(bytes(300), 16300, ref.POLY["crc32"]) == zlib.crc32(bytes(300))


def test_adler_overflow_cases():
    for data in (b"\xff" * 5552, b"\xff" * 5553, b"\x01" * 65521, b"\xff" * (1 << 20 | 1)):
        assert ref.adler_in_pieces(data, [len(data) // 3, len(data) // 2]) == zlib.adler32(data)


# ---- the layout builder ----------------------------------------------------------------------------------------------------
def _record_inputs(modalities):
    from acimg import convert
    rng = np.random.RandomState(21)
    rec = convert.Recording("d", 7, 12, 1, "v", "w")
    audio = rng.randint(-2 ** 31, 2 ** 31 - 1, (12, 1024), dtype=np.int64).astype(np.int32)
    video = rng.randint(0, 256, (12, 5, 7, 3)).astype(np.uint8)          # small fake frames
    return rec, (audio if modalities is None or 1 in modalities else None), (video if modalities is None or 2 in modalities else None)


@pytest.mark.parametrize("modalities", [None, (1,), (2,), (1, 2)], ids=["all", "audio", "video", "audio+video"])
def test_layout_equals_the_framed_record(lib, tmp_path, modalities):
    import gzip

    from acimg import convert, tfio
    rec, audio, video = _record_inputs(modalities)
    want = tfio.frame_record(convert.build_record(rec, audio, video))
    lay = convert.build_record_layout(rec, audio, 5 * 7 * 3, None if video is None else video.shape)
    assert len(lay.skeleton) == len(want) and lay.data == (12, len(want) - 16) and lay.trailer == len(want) - 4
    assert len(lay.holes) == (0 if video is None else 12) and all(n == 105 for _, n in lay.holes)
    assert lay.skeleton[:12] == want[:12] and lay.skeleton[-4:] == bytes(4)
    for off, n in lay.holes:
        assert lay.skeleton[off:off + n] == bytes(n)
    covered = sorted(lay.pieces() + lay.holes + [(lay.trailer, 4)])
    assert covered[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(covered, covered[1:] + [(len(want), 0)]))
    for off, n in lay.pieces():
        assert n > 0 and lay.skeleton[off:off + n] == want[off:off + n]
    got = lay.fill([] if video is None else [f.tobytes() for f in video])
    assert got == want
    path = tmp_path / "r.tfrecord"
    path.write_bytes(gzip.compress(got))
    (back,) = list(tfio.read_tfrecord(str(path), "GZIP", verify=True))
    assert back == want[12:-4]


def test_layout_of_single_values_and_mixed_lists(lib):
    from collections import OrderedDict

    from acimg import tfio
    ctx = OrderedDict((("a", b"xyz"), ("big", tfio.External(300)), ("n", np.array([1, 2, 300]))))
    lists = OrderedDict((("l", [[b"in", tfio.External(5)], np.array([1.5, 2.5], np.float32)]),))
    lay = tfio.build_record_layout(ctx, lists)
    big, five = bytes(range(256)) + bytes(44), b"\x01\x02\x03\x04\x05"
    ctx["big"] = big
    lists["l"][0] = [b"in", five]
    assert lay.fill([big, five]) == tfio.frame_record(tfio.build_sequence_example(ctx, lists))
    with pytest.raises(ValueError):
        lay.fill([big])


# ---- refusals before any launch --------------------------------------------------------------------------------------------
_BIG = (C.c_char * 8192)()
A = C.addressof(_BIG) + (-C.addressof(_BIG)) % 256          # a fake, 256-byte aligned "device pointer": never dereferenced


def test_version_and_workspace_arithmetic(lib):
    assert lib.acimg_version() == 207
    q = lib.acimg_checksum_workspace
    up = lambda v: -(-v // 16) * 16      # noqa: E731
    for total, count in ((0, 1), (1, 1), (16384, 1), (3 * 16384 + 5, 4), (2 ** 31 - 1, 1), (10 * (2 ** 31 - 1), 10)):
        segs = total // ref.SEGMENT + 2 * count
        assert q(total, count) == up(24 * segs) + up(24 * count) + up(8 * segs), (total, count)
    assert q(-1, 1) == 0 and q(5, 0) == 0
    g = lib.acimg_record_gather_workspace
    assert g(0) == 0 and g(-3) == 0 and g(1) == 32 and g(7) == 224


def test_checksum_refusals(lib):
    from acimg import _lib
    ws = lib.acimg_checksum_workspace(100, 2)

    def call(lengths=(60, 40), kind=0, in_=A, out=A, ws_ptr=A, ws_bytes=ws, store_base=None, store_at=None, count=None):
        n = len(lengths) if count is None else count
        return lib.acimg_checksum(in_, ref.longs(*lengths) if lengths else None, n, kind, out, store_base, store_at, ws_ptr, ws_bytes, None)
    assert call(kind=4) == EINVAL and "kind" in _lib.last_error()
    assert call(kind=-1) == EINVAL
    assert call(lengths=(60, -1)) == EINVAL and "payload 1" in _lib.last_error()
    assert call(lengths=(2 ** 31, 40), ws_bytes=1 << 30) == EINVAL and "payload 0" in _lib.last_error()
    assert call(ws_bytes=ws - 16) == EWORKSPACE
    assert call(count=0) == EINVAL
    assert call(in_=None) == EINVAL and call(out=None) == EINVAL and call(ws_ptr=None) == EINVAL
    assert call(lengths=None, count=2) == EINVAL
    assert call(ws_ptr=A + 8) == EINVAL and "aligned" in _lib.last_error()
    assert call(store_at=ref.longs(0, -1)) == EINVAL and "store_base" in _lib.last_error()


def test_record_gather_refusals(lib):
    from acimg import _lib

    def call(rows, dst_bytes=1000, src0=A, src1=A, dst=A, ws_ptr=A, ws_bytes=None):
        flat = [v for r in rows for v in r]
        need = lib.acimg_record_gather_workspace(len(rows))
        return lib.acimg_record_gather(src0, src1, ref.longs(*flat) if flat else None, len(rows), dst, dst_bytes, ws_ptr,
                                       need if ws_bytes is None else ws_bytes, None)
    ok = [(0, 0, 10, 0), (10, 5, 20, 1)]
    assert call(ok, ws_bytes=lib.acimg_record_gather_workspace(2) - 16) == EWORKSPACE
    assert call([(0, 0, 10, 0), (9, 0, 5, 1)]) == EINVAL and "overlap" in _lib.last_error()
    assert call([(20, 0, 10, 0), (0, 0, 5, 0), (4, 0, 3, 1)]) == EINVAL and "overlap" in _lib.last_error()
    assert call([(995, 0, 6, 0)]) == EINVAL and "outside" in _lib.last_error()
    assert call([(1001, 0, 0, 0)]) == EINVAL
    assert call([(-1, 0, 4, 0)]) == EINVAL and call([(0, -1, 4, 0)]) == EINVAL and call([(0, 0, -4, 0)]) == EINVAL
    assert call([(0, 0, 4, 2)]) == EINVAL and "source" in _lib.last_error()
    assert call([(0, 0, 4, 1)], src1=None) == EINVAL and "null" in _lib.last_error()
    assert call([]) == EINVAL
    assert call(ok, dst=None) == EINVAL and call(ok, ws_ptr=None) == EINVAL and call(ok, ws_ptr=A + 4) == EINVAL


# ---- the switch ------------------------------------------------------------------------------------------------------------
def test_assemble_device_needs_deflate_device(lib, tmp_path):
    from acimg import convert
    with pytest.raises(convert.ConvertError, match="--deflate device"):
        convert.Converter(str(tmp_path), deflate="zlib", assemble="device")
    with pytest.raises(convert.ConvertError, match="--deflate device"):
        convert.convert(str(tmp_path), str(tmp_path), assemble="device")
    with pytest.raises(convert.ConvertError, match="--assemble"):
        convert.Converter(str(tmp_path), assemble="gpu")
    args = convert.build_parser().parse_args([str(tmp_path), str(tmp_path)])
    assert args.assemble == "host" and convert.ASSEMBLE_CHOICES == ("host", "device")
    with pytest.raises(convert.ConvertError, match="--deflate device"):
        convert.main([str(tmp_path), str(tmp_path), "--assemble", "device"])
    assert os.listdir(str(tmp_path)) == []
