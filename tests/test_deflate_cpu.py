"""The device DEFLATE encoder without a GPU: the restatement (tests/deflate_ref.py - the device's parse rule, code
construction and header choices) against zlib's own decoder on every payload of tests/deflate_cases.py; the containers of
acimg.deflate against `gzip` / `zlib`; the code construction's properties on synthetic histograms; the refusals of the C
entry points with fake pointers (a call that fails to refuse reaches a launch and comes back as ACIMG_ELAUNCH here); and the
default (zlib) paths of `write_tfrecord` / `encode_png`, which must write what they always wrote."""
import ctypes as C
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import deflate_cases as cases  # noqa: E402
import deflate_ref as ref  # noqa: E402

EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


# ---- 1 streams -------------------------------------------------------------------------------------------------------------
def test_block_constant_is_one():
    from acimg import deflate
    assert deflate.BLOCK == ref.BLOCK and deflate.BLOCK in (16384, 32768, 65536)
    assert deflate.EMPTY_STREAM == ref.EMPTY_FINAL == ref.deflate(b"")
    assert zlib.decompress(deflate.EMPTY_STREAM, -15) == b""


@pytest.mark.parametrize("name,payload", cases.PAYLOADS, ids=[n for n, _ in cases.PAYLOADS])
def test_restated_stream_inflates_to_the_payload(name, payload):
    from acimg import deflate
    stream = ref.deflate(payload)
    assert zlib.decompress(stream, -15) == payload
    assert len(stream) <= deflate.bound(len(payload)) == ref.bound(len(payload))
    assert gzip.decompress(deflate.gzip_container(stream, payload)) == payload
    assert zlib.decompress(deflate.zlib_container(stream, payload)) == payload


def test_containers_carry_their_fields():
    from acimg import deflate
    payload = b"records " * 100
    stream = ref.deflate(payload)
    g = deflate.gzip_container(stream, payload)
    assert g[:10] == b"\x1f\x8b\x08\x00" + b"\x00" * 4 + b"\x00\xff" and g[10:-8] == stream       # mtime 0
    assert int.from_bytes(g[-8:-4], "little") == zlib.crc32(payload) and int.from_bytes(g[-4:], "little") == len(payload)
    z = deflate.zlib_container(stream, payload)
    assert z[:2] == b"\x78\x01" and z[2:-4] == stream and int.from_bytes(z[-4:], "big") == zlib.adler32(payload)
    with pytest.raises(zlib.error):
        zlib.decompress(z[:-1] + bytes([z[-1] ^ 1]))


def test_parse_takes_no_match_across_a_block_and_none_below_three():
    payload = dict(cases.PAYLOADS)["second_block_repeats_first"]
    # each block alone is noise: both are stored, although the second repeats the first
    assert len(ref.deflate(payload)) == len(payload) + 5 + 5 + 5
    assert ref.greedy_parse(np.frombuffer(b"\x41\x41", np.uint8)) == [(0, 0, 0), (1, 0, 0)]
    toks = ref.greedy_parse(np.zeros(ref.BLOCK, np.uint8))
    assert toks[0] == (0, 0, 0) and toks[1] == (1, 258, 1) and all(d == 1 for _, l, d in toks[1:])
    assert sum(l if l else 1 for _, l, _ in toks) == ref.BLOCK


# ---- 2 code construction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsym,limit", cases.ALPHABETS)
def test_code_lengths_on_synthetic_histograms(nsym, limit):
    rows = cases.histogram_rows(nsym)
    limited = 0
    for r, row in enumerate(rows):
        lengths = ref.huffman_lengths(row, limit)
        depth = cases.check_lengths(row, lengths, limit, "row %d" % r)
        limited += depth > limit
    # Fibonacci counts: n symbols give an unlimited depth of n - 1, so the limiter acts on 17 and 19 symbols at limit 15 and
    # on 9, 17 and 19 at limit 7
    assert limited == (2 if limit == 15 else 3)
    assert not any(ref.huffman_lengths(rows[-1], limit))
    assert sorted(set(ref.huffman_lengths(rows[-2], limit))) in ([8, 9], [4, 5])      # all equal: two adjacent lengths


def test_code_lengths_on_random_histograms():
    rng = np.random.RandomState(3)
    for nsym, limit in cases.ALPHABETS:
        for trial in range(300):
            row = np.zeros(nsym, np.int64)
            k = rng.randint(1, nsym + 1)
            where = rng.permutation(nsym)[:k]
            row[where] = (2.0 ** rng.uniform(0, 24 if trial % 2 else 3, k)).astype(np.int64)
            cases.check_lengths(row, ref.huffman_lengths(row, limit), limit, "%d symbols, trial %d" % (nsym, trial))


def test_canonical_codes_are_prefix_free():
    lengths = ref.huffman_lengths(cases.histogram_rows(30)[4], 15)
    codes = ref.canonical_codes(lengths)
    words = sorted(format(c, "0%db" % l)[::-1] for c, l in zip(codes, lengths) if l)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))


# ---- 3 the C entry points ----------------------------------------------------------------------------------------------------
_BIG = (C.c_char * 8192)()
A = C.addressof(_BIG) + (-C.addressof(_BIG)) % 256          # a fake, 256-byte aligned "device pointer": never dereferenced


def _error(lib):
    from acimg import _lib
    return _lib.last_error()


def test_bound_and_workspace_queries(lib):
    from acimg import deflate
    B = deflate.BLOCK
    assert lib.acimg_version() == 207
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 17, 10 ** 9):
        assert lib.acimg_deflate_bound(n) == n + 10 * -(-n // B) + 5 == deflate.bound(n)
    assert lib.acimg_deflate_bound(-1) == 0
    per_block = 24 + 4 + 8 + B + 16
    assert lib.acimg_deflate_workspace(0, 1) == 0 and lib.acimg_deflate_workspace(5, 0) == 0
    assert lib.acimg_deflate_workspace(3, 4) == 0                                      # every payload has a byte
    for total, count in ((1, 1), (B, 1), (3 * B + 17, 1), (5 * B, 4)):
        blocks = total // B + count
        got = lib.acimg_deflate_workspace(total, count)
        assert blocks * per_block <= got <= blocks * per_block + 3 * 16, (total, count, got)


def test_deflate_refusals_come_before_any_launch(lib):
    from acimg import deflate
    B = deflate.BLOCK
    one = (C.c_long * 1)(3 * B + 17)
    out_bytes, ws = lib.acimg_deflate_bound(3 * B + 17), lib.acimg_deflate_workspace(3 * B + 17, 1)

    def call(inp=A, lengths=one, count=1, out=A, nout=out_bytes, sizes=A, w=A, nws=ws):
        return lib.acimg_deflate(inp, lengths, count, out, nout, sizes, w, nws, None)

    for kw in (dict(inp=None), dict(lengths=None), dict(out=None), dict(sizes=None), dict(w=None)):
        assert call(**kw) == EINVAL and "null" in _error(lib), kw
    assert call(count=0) == EINVAL and "count" in _error(lib)
    assert call(count=-3) == EINVAL
    assert call(lengths=(C.c_long * 1)(0)) == EINVAL and "0 bytes" in _error(lib)
    assert call(lengths=(C.c_long * 1)(-5)) == EINVAL and "-5 bytes" in _error(lib)
    assert call(lengths=(C.c_long * 2)(B, -1), count=2) == EINVAL and "payload 1" in _error(lib)
    assert call(nout=out_bytes - 1) == EINVAL and "out_bytes" in _error(lib)
    two = (C.c_long * 2)(B + 1, 7)
    need = lib.acimg_deflate_bound(B + 1) + lib.acimg_deflate_bound(7)
    assert call(lengths=two, count=2, nout=need - 1, nws=lib.acimg_deflate_workspace(B + 8, 2)) == EINVAL
    assert call(w=A + 8) == EINVAL and "aligned" in _error(lib)
    assert call(nws=ws - 1) == EWORKSPACE and "workspace" in _error(lib)
    assert call(nws=0) == EWORKSPACE


def test_huffman_lengths_refusals_come_before_any_launch(lib):
    def call(freq=A, n=1, nsym=19, limit=7, out=A):
        return lib.acimg_huffman_lengths(freq, n, nsym, limit, out, None)

    assert call(freq=None) == EINVAL and "null" in _error(lib)
    assert call(out=None) == EINVAL
    assert call(n=0) == EINVAL and "n = 0" in _error(lib)
    assert call(nsym=0) == EINVAL and call(nsym=289) == EINVAL and "nsym" in _error(lib)
    assert call(limit=0) == EINVAL and call(limit=16) == EINVAL and "limit" in _error(lib)
    assert call(nsym=19, limit=4) == EINVAL                                             # 16 codes of 4 bits at most


# ---- 4 the default paths ------------------------------------------------------------------------------------------------------
def test_write_tfrecord_without_a_deflater_is_gzip_open(tmp_path):
    from acimg import tfio
    records = [b"first record", bytes(range(256)) * 40, b""]
    framed = b"".join(tfio.frame_record(r) for r in records)
    tfio.write_tfrecord(str(tmp_path / "plain.tfrecord"), records)
    assert (tmp_path / "plain.tfrecord").read_bytes() == framed
    tfio.write_tfrecord(str(tmp_path / "gz.tfrecord"), records, compression="GZIP")
    data = (tmp_path / "gz.tfrecord").read_bytes()
    assert gzip.decompress(data) == framed
    # gzip.open's own stream: level 9, written record by record
    co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY)
    body = b"".join(co.compress(tfio.frame_record(r)) for r in records) + co.flush()
    assert data[10 + len(b"gz.tfrecord") + 1:-8] == body
    assert list(tfio.read_tfrecord(str(tmp_path / "gz.tfrecord"))) == records


def test_write_tfrecord_with_a_deflater_writes_one_member(tmp_path):
    from acimg import deflate, tfio

    class Restated(object):                     # the device's streams, from the restatement
        def gzip(self, data):
            return deflate.gzip_container(ref.deflate(data), data)

    records = [b"first record", bytes(range(256)) * 40]
    path = str(tmp_path / "dev.tfrecord")
    tfio.write_tfrecord(path, records, compression="GZIP", deflater=Restated())
    assert list(tfio.read_tfrecord(path)) == records
    tfio.write_tfrecord(path, records, deflater=Restated())                 # no compression asked: none done
    assert open(path, "rb").read() == b"".join(tfio.frame_record(r) for r in records)


def test_encode_png_without_a_deflater_is_zlib_compress():
    from acimg import deflate, png
    rng = np.random.RandomState(2)
    img = (np.arange(7 * 5 * 3).reshape(7, 5, 3) * 3 + rng.randint(0, 4, (7, 5, 3))).astype(np.uint8)
    rows = np.concatenate([np.zeros((7, 1), np.uint8), img.reshape(7, 15)], 1).tobytes()
    for level in (1, 6):
        data = png.encode_png(img, level)
        idat = zlib.compress(rows, level)
        assert data[:8] == png.SIGNATURE and data[33:41] == len(idat).to_bytes(4, "big") + b"IDAT"
        assert data[41:41 + len(idat)] == idat and len(data) == 41 + len(idat) + 4 + 12

    class Restated(object):
        def zlib(self, data):
            return deflate.zlib_container(ref.deflate(data), data)

    data = png.encode_png(img, deflater=Restated())
    n = int.from_bytes(data[33:37], "big")
    assert zlib.decompress(data[41:41 + n]) == rows


def test_the_tools_take_the_switch_and_default_to_zlib():
    from acimg import convert, convert_boxes, show
    for mod in (convert, convert_boxes):
        p = mod.build_parser()
        assert p.get_default("deflate") == "zlib"
        with pytest.raises(SystemExit):
            p.parse_args([HERE, HERE, "--deflate", "lz4"])
        assert p.parse_args([HERE, HERE, "--deflate", "device"]).deflate == "device"
    assert convert.make_deflater("zlib", "cuda:0") is None
    with pytest.raises(convert.ConvertError):
        convert.make_deflater("lz4", "cuda:0")
    common = ["--train_file", "x", "--init_checkpoint", "y"]
    assert show.build_parser().parse_args(["video"] + common).png_deflate == "zlib"
    assert show.build_parser().parse_args(["boxes"] + common + ["--png_deflate", "device"]).png_deflate == "device"
