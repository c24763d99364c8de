"""The device inflater without a GPU: the restatement (tests/inflate_ref.py - the finder's rule, the count pass and its stop
rule, the chain, the markers and both resolve steps) against zlib on every stream of tests/inflate_cases.py at every chunk
size; what the finder finds; that the chunks really decode side by side (the coverage condition); that the streams reach
every rare path of RFC 1951 the decoder has code for, in chunks that start live (tests/inflate_census.py); corrupt and truncated
input with the right status; `parse_gzip`; the refusals of the C entry point with fake pointers (a call that fails to
refuse reaches a launch and comes back as ACIMG_ELAUNCH here); and the loader's argument check."""
import ctypes as C
import gzip
import os
import sys
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import inflate_cases as cases  # noqa: E402
import inflate_census as census  # noqa: E402
import inflate_ref as ref  # noqa: E402

EINVAL, EWORKSPACE = -1, -2
BY_NAME = {name: (stream, payload) for name, stream, payload in cases.CASES}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


# ---- 1 the restatement against zlib -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in cases.CASES])
def test_restatement_equals_zlib(name):
    stream, payload = BY_NAME[name]
    tail = zlib.decompressobj(-15)
    assert tail.decompress(stream) == payload and tail.eof and tail.unused_data == b""
    for chunk in cases.CHUNKS:
        r = ref.inflate(stream, len(payload), chunk)
        assert r.status == ref.OK and r.out == payload, (name, chunk, r.status)
        assert (r.end_bits + 7) // 8 == len(stream), (name, chunk)
        assert r.live[0] == 1 and r.offsets[0] == 0
        assert sum(n for n, live in zip(r.lengths, r.live) if live) == len(payload)
        assert len(r.starts) == max(1, -(-len(stream) // chunk))


# ---- 2 the finder -------------------------------------------------------------------------------------------------------------
FINDER_CASES = ("smooth-mem1", "smooth64k-mem1", "tone_int32-mem1_level9", "smooth_noise-sync_flush", "window_spanning",
                "zeros_then_smooth-device_encoder", "random-level0", "smooth-fixed", "deep_codes", "run_crosses_alphabets",
                "stored_edges")


@pytest.mark.parametrize("name", FINDER_CASES)
def test_finder_finds_every_true_start_that_is_its_chunks_lowest_hit(name):
    stream, payload = BY_NAME[name]
    headers = ref.block_headers(stream, len(payload))
    true_starts = [bit for bit, final, btype in headers if btype == 2 and not final]
    for bit in true_starts:
        assert ref.is_start(stream, bit), (name, bit)
    for bit, final, btype in headers:
        if btype != 2 or final:
            assert not ref.is_start(stream, bit), (name, bit, btype)     # only dynamic, non-final headers are sought
    for chunk in (256, 1024):
        starts = ref.find_starts(stream, chunk)
        for j in range(1, len(starts)):
            inside = [b for b in true_starts if 8 * j * chunk <= b < 8 * (j + 1) * chunk]
            if inside:                       # a hit below the first true start is a false one: the chain will not take it
                assert 8 * j * chunk <= starts[j] <= inside[0], (name, chunk, j)
            if starts[j] >= 0:
                assert ref.is_start(stream, starts[j])
                assert not any(ref.is_start(stream, o) for o in range(max(8 * j * chunk, starts[j] - 64), starts[j]))


def test_chunks_decode_side_by_side():
    """the coverage condition: on the 64 KiB smooth image at level 6, memLevel 1, chunk_bytes 1024 at least three quarters of
    the chunks after the first are live - the tests cannot pass with everything decoded by chunk 0"""
    stream, payload = BY_NAME[cases.COVERAGE_CASE]
    r = ref.inflate(stream, len(payload), 1024)
    later = r.live[1:]
    print("%d of %d chunks after the first are live; %d blocks" % (sum(later), len(later),
                                                                     len(ref.block_headers(stream, len(payload)))))
    assert len(later) >= 12 and 4 * sum(later) >= 3 * len(later)
    assert all(s >= 0 for s, live in zip(r.starts, r.live) if live)
    # every live start is a true block boundary
    true_bits = {bit for bit, _, _ in ref.block_headers(stream, len(payload))}
    assert all(s in true_bits for s, live in zip(r.starts, r.live) if live)


def test_false_start_is_found_and_left_dead():
    stream, payload = BY_NAME["false_start"]
    r = ref.inflate(stream, len(payload), cases.GPU_CHUNK)
    assert r.starts[1] == 8 * cases.GPU_CHUNK and r.live == [1] + [0] * (len(r.live) - 1)
    assert r.status == ref.OK and r.out == payload


def test_markers_reach_back_over_several_short_chunks():
    stream, payload = BY_NAME["window_spanning"]
    r = ref.inflate(stream, len(payload), 256)
    live = [n for n, l in zip(r.lengths, r.live) if l]
    assert len(live) >= 4 and max(live[1:]) < ref.WINDOW
    assert r.marker_reach >= 3, r.marker_reach
    assert r.out == payload


# ---- 2a what the streams reach of the format ------------------------------------------------------------------------------------
CENSUS_ROWS = (("longest literal/length code decoded", "ll_bits", max), ("longest distance code decoded", "d_bits", max),
               ("HCLEN", "hclen", max), ("blocks with all 19 code-length lengths, the last one non-zero", "cl_symbol_15", sum),
               ("longest code of a code-length code", "cl_bits", max), ("length 258 as symbol 284 + extra 31", "len258_as_284", sum),
               ("length 258 as symbol 285", "len258_as_285", sum), ("largest distance", "dist_max", max),
               ("copies at distance 32768", "dist_32768", sum), ("largest LEN of a stored block", "stored_len_max", max),
               ("blocks with HLIT = HDIST = 29", "hlit29_hdist29", sum))


def _placed(name, chunk):
    stream, payload = BY_NAME[name]
    return census.place_in_chunks(census.walk(stream), ref.inflate(stream, len(payload), chunk))


def _copies(blocks):
    return [(b, t) for b in blocks for t in b.tokens if t.literal is None]


def test_the_cases_reach_every_listed_feature():
    """every rare path of RFC 1951 that the device decoder has code for is reached by a stream of CASES, and reached where it
    matters: in chunks that start live, not only in the serial decode of chunk 0.  Each condition names its stream, so
    taking a stream away fails here."""
    token = {name for name, _ in cases.TOKEN_CASES}
    counted = {name: census.census(stream) for name, stream, _ in cases.CASES}
    print()
    total = {}
    for title, key, fold in CENSUS_ROWS:
        before = fold(c[key] for name, c in counted.items() if name not in token)
        total[key] = fold(c[key] for c in counted.values())
        print("%-66s %6d -> %6d" % (title, before, total[key]))
    crossing = sorted(set(x for c in counted.values() for x in c["crossing"]))
    print("%-66s %s -> %s" % ("repeat runs (symbol, value) over the boundary of the two alphabets",
                              sorted(set(x for n, c in counted.items() if n not in token for x in c["crossing"])), crossing))
    assert (total["ll_bits"], total["d_bits"], total["hclen"], total["cl_bits"]) == (15, 15, 15, 7) and total["cl_symbol_15"] > 0
    assert total["len258_as_284"] > 0 and total["len258_as_285"] > 0
    assert total["dist_max"] == 32768 and total["dist_32768"] >= 3 and total["stored_len_max"] == 65535

    # deep_codes
    blocks = _placed("deep_codes", 256)
    deep = [b for b in blocks if b.btype == 2]
    assert len([b for b in deep if not b.final]) >= 4 and deep[-1].final and deep[-1] is blocks[-1]
    assert blocks[blocks.index(deep[0]):] == deep                                    # consecutive
    for b, nxt in zip(deep, deep[1:] + [None]):
        assert (nxt.bit if nxt else b.end) - b.bit > 8 * 256, b.bit
        assert {14, 15} <= {t.ll_bits for t in b.tokens}
        assert {10, 11, 12, 13, 14, 15} <= {t.d_bits for t in b.tokens if t.literal is None}
        assert b.hclen == 15 and b.cl[15] and max(b.cl) == 7
    r = ref.inflate(BY_NAME["deep_codes"][0], len(BY_NAME["deep_codes"][1]), 256)
    assert {r.starts[j] for j, l in enumerate(r.live) if l} <= {b.bit for b in blocks}      # true block boundaries
    started = [b for b in deep if b.chunk >= 1 and b.starts_chunk]
    assert len(started) >= 4 and len({b.chunk for b in started}) == len(started)
    for b in started:
        assert any(t.ll_bits == 15 for t in b.tokens) and any(t.d_bits >= 14 for t in b.tokens if t.literal is None)
    markers = [t for b, t in _copies(started) if t.d_bits == 15 and t.dist > t.produced]
    print("deep_codes: %d blocks, %d of them start a live chunk at chunk_bytes 256; %d copies through a 15-bit distance code "
          "write markers" % (len(deep), len(started), len(markers)))
    assert markers

    # run_crosses_alphabets
    runs = [b.crossing for b in census.walk(BY_NAME["run_crosses_alphabets"][0]) if b.btype == 2]
    assert sorted(x[0] for run in runs for x in run) == [16, 17, 18] and all(len(run) == 1 for run in runs)
    assert [x for run in runs for x in run if x[0] == 16][0][1] > 0                   # a non-zero length is carried across
    assert counted["run_crosses_alphabets"]["hlit29_hdist29"] >= 1
    blocks = _placed("run_crosses_alphabets", 256)
    assert all(b.chunk >= 1 and b.starts_chunk for b in blocks if b.btype == 2)      # so the finder reads these headers too

    # far_and_long
    blocks = _placed("far_and_long", 256)
    far = [(b, t) for b, t in _copies(blocks) if t.dist == 32768]
    stored = [b for b in blocks if b.btype == 0]
    assert any(b.chunk == 0 and t.out == 32768 for b, t in far)                       # dist == produced in chunk 0
    assert any(b.chunk >= 1 and b.starts_chunk for b, t in far)
    assert any(s.out <= t.out - 32768 and t.out - 32768 + t.length <= s.out + s.ln for b, t in far for s in stored)
    long = [t for b, t in _copies(blocks) if t.length == 258]
    assert {284, 285} == {t.symbol for t in long}
    assert {1, 2, 63, 64, 65, 257} <= {t.dist for t in long if t.symbol == 285}
    assert {1, 2, 63, 64, 65, 257} <= {t.dist for t in long if t.symbol == 284}
    assert {1, 2, 63, 64, 65, 257} <= {t.dist for b, t in _copies(blocks) if t.length == 258 and b.chunk >= 1}

    # copy_straddles_chunk_start
    for chunk in (256, 1024):
        blocks = _placed("copy_straddles_chunk_start", chunk)
        straddle = [t for b, t in _copies(blocks) if b.chunk >= 1 and b.starts_chunk and t.produced < t.dist < t.produced + t.length]
        assert any(t.dist >= t.length for t in straddle) and any(t.dist < t.length for t in straddle), chunk

    # literal_runs
    runs = set(census.runs_of_literals(census.walk(BY_NAME["literal_runs"][0])))
    print("literal_runs:", sorted(runs))
    assert {(n, end) for n in cases.LITERAL_RUNS for end in ("copy", "eob", "stored")} <= runs and (63, "end") in runs

    # stored_edges
    blocks = _placed("stored_edges", 256)
    big = census.walk(BY_NAME["stored_edges-len_65535"][0])
    assert any(b.btype == 0 and b.ln == 65535 for b in big)
    assert any(b.btype == 0 and b.ln == 0 and a.btype == 2 and c.btype == 2 for a, b, c in zip(blocks, blocks[1:], blocks[2:]))
    assert {b.bit % 8 for b in blocks if b.btype == 0} == set(range(8))
    assert any(a.btype == 0 and a.end % (8 * 256) == 0 and b.btype == 2 and not b.final and b.starts_chunk
               and b.bit == 8 * 256 * b.chunk for a, b in zip(blocks, blocks[1:]))
    ends = [bl[-1] for bl in (blocks, big)]
    assert all(b.final and b.btype == 1 for b in ends) and sorted(b.end % 8 for b in ends) == [0, 1]      # no pad bit; 7


def test_zlib_refuses_the_token_level_corrupt_streams():
    listed = {c[0]: c for c in cases.corrupt_streams()}
    for name, stream, size in cases.token_corrupt_streams():
        _zlib_refuses(stream)
        for chunk in (256, 1 << 22):
            assert ref.inflate(stream, size, chunk).status == listed[name][3] != ref.OK, name
    assert listed["cut_inside_a_15_bit_code"][3] == ref.TRUNCATED
    assert all(listed[n][3] == ref.CORRUPT for n, _, _ in cases.token_corrupt_streams()[:-1])


# ---- 3 corrupt input ------------------------------------------------------------------------------------------------------------
def _hand(**kw):
    return cases.dynamic_block(cases.BitWriter(), **kw).bytes()


def _zlib_refuses(stream):
    with pytest.raises(zlib.error):
        zlib.decompress(stream, -15)


def test_the_hand_made_block_is_valid():
    stream = _hand()
    assert zlib.decompress(stream, -15) == b"aaa"
    r = ref.inflate(stream, 3, 256)
    assert (r.status, r.out, r.end_bits) == (ref.OK, b"aaa", cases.dynamic_block(cases.BitWriter()).n)


BROKEN = cases.BROKEN_HEADERS


@pytest.mark.parametrize("name,kw", BROKEN, ids=[b[0] for b in BROKEN])
def test_each_broken_header_field_is_corrupt(name, kw):
    stream = _hand(**kw) + bytes(8)             # zero bytes behind it: nothing is truncated
    _zlib_refuses(stream)
    for chunk in (256, 1 << 22):
        assert ref.inflate(stream, 3, chunk).status == ref.CORRUPT, name
    assert not ref.is_start(_hand(final=0, **kw) + bytes(8), 0)


def test_distance_before_the_stream_and_len_nlen():
    w = cases.BitWriter().bits(1, 1).bits(1, 2)                 # a fixed block: literal 'a', then length 3 at distance 2
    w.code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7)
    stream = w.bytes()
    _zlib_refuses(stream)
    assert ref.inflate(stream, 4, 256).status == ref.CORRUPT
    good = cases.BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 97, 8).code(1, 7).code(0, 5).code(0, 7).bytes()
    assert zlib.decompress(good, -15) == b"aaaa" and ref.inflate(good, 4, 256).out == b"aaaa"
    stored = cases.BitWriter().bits(1, 1).bits(0, 2).align().bits(5, 16).bits(~5 ^ 1, 16).raw(b"hello").bytes()
    _zlib_refuses(stored)
    assert ref.inflate(stored, 5, 256).status == ref.CORRUPT


def _short_streams():
    smooth = cases.smooth_ramp(3).tobytes()
    rnd = BY_NAME["random-level0"][1][:300]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    fixed = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    return [("dynamic_blocks", co.compress(smooth) + co.flush(), smooth),
            ("stored", zlib.compress(rnd, 0)[2:-4], rnd),
            ("fixed", fixed.compress(smooth[:400]) + fixed.flush(), smooth[:400]),
            ("single_length_one_code",) + BY_NAME["single_length_one_code"]]


@pytest.mark.parametrize("name,stream,payload", _short_streams(), ids=[c[0] for c in _short_streams()])
def test_truncation_at_every_byte(name, stream, payload):
    assert zlib.decompress(stream, -15) == payload and ref.inflate(stream, len(payload), 256).status == ref.OK
    assert len(stream) < 1200
    for n in range(1, len(stream)):
        r = ref.inflate(stream[:n], len(payload), 256)
        assert r.status == ref.TRUNCATED, (name, n, r.status)
        d = zlib.decompressobj(-15)
        d.decompress(stream[:n])
        assert not d.eof


@pytest.mark.parametrize("name", ["smooth-mem1", "random-level0", "one_byte-level6"])
def test_a_wrong_expected_size_both_ways(name):
    stream, payload = BY_NAME[name]
    for chunk in (256, 1 << 22):
        assert ref.inflate(stream, len(payload) + 1, chunk).status == ref.SIZE
        if len(payload) > 1:
            assert ref.inflate(stream, len(payload) - 1, chunk).status == ref.SIZE
        assert ref.inflate(stream, len(payload), chunk).status == ref.OK


def test_the_corrupt_streams_of_the_gpu_test_fail_as_listed():
    for name, stream, size, status in cases.corrupt_streams():
        got = ref.inflate(stream, size, cases.GPU_CHUNK).status
        assert got == status != ref.OK, (name, got, status)
        try:
            assert zlib.decompress(stream, -15) != b"" and status == ref.SIZE, name        # zlib itself knows no expected size
        except zlib.error:
            pass


# ---- 4 containers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", range(32))
def test_parse_gzip_on_every_flag_combination(flags):
    from acimg import inflate
    payload = b"records " * 40
    body = zlib.compress(payload, 6)[2:-4]
    head = bytes([0x1F, 0x8B, 8, flags, 1, 2, 3, 4, 0, 255])
    if flags & inflate.FEXTRA:
        head += (7).to_bytes(2, "little") + b"AB\x03\x00xyz"
    if flags & inflate.FNAME:
        head += b"part0.tfrecord\x00"
    if flags & inflate.FCOMMENT:
        head += b"a comment\x00"
    if flags & inflate.FHCRC:
        head += (zlib.crc32(head) & 0xFFFF).to_bytes(2, "little")
    raw = head + body + (zlib.crc32(payload) & 0xFFFFFFFF).to_bytes(4, "little") + len(payload).to_bytes(4, "little")
    assert gzip.decompress(raw) == payload
    off, length, crc, isize = inflate.parse_gzip(raw)
    assert (off, length, crc, isize) == (len(head), len(body), zlib.crc32(payload), len(payload))
    assert raw[off:off + length] == body and inflate.gzip_plan(raw) == (off, length, crc, isize)
    r = ref.inflate(body, isize, 256)
    assert r.out == payload and (r.end_bits + 7) // 8 == length


def test_parse_gzip_refuses_what_is_no_member():
    from acimg import inflate
    good = gzip.compress(b"abc")
    for bad in (b"", good[:17], b"\x1f\x8c" + good[2:], good[:2] + b"\x07" + good[3:], good[:3] + b"\x20" + good[4:],
                good[:3] + b"\x08" + good[4:10] + b"name-without-end"):
        with pytest.raises(ValueError):
            inflate.parse_gzip(bad)
        assert inflate.gzip_plan(bad) is None
    empty = gzip.compress(b"")
    assert inflate.parse_gzip(empty)[3] == 0 and inflate.gzip_plan(empty) is None       # ISIZE 0: the host's


# ---- 5 the C entry ------------------------------------------------------------------------------------------------------------------
_BIG = C.create_string_buffer(1 << 16)
A = C.addressof(_BIG) + (-C.addressof(_BIG)) % 256          # a fake, 256-byte aligned "device pointer": never dereferenced


def _last_error(lib):
    buf = C.create_string_buffer(512)
    lib.acimg_last_error(buf, 512)
    return buf.value.decode()


def test_workspace_query(lib):
    from acimg import inflate
    q = lib.acimg_inflate_workspace
    r16 = lambda v: (v + 15) & ~15      # noqa: E731
    item = inflate.CHUNK_DTYPE.itemsize
    assert q(1000, 5000, 1, 256) == r16((1000 // 256 + 1) * item) + r16(4) + r16(2 * 5000)
    assert q(70000, 3, 3, 32768) == r16((2 + 3) * item) + r16(12) + 16
    for bad in ((0, 1, 1, 256), (1, 0, 1, 256), (10, 10, 0, 256), (10, 10, 11, 256), (10, 10, 1, 255), (10, 10, 1, 128),
                (10, 10, 1, 768), (10, 10, 1, 1 << 25), (10, 10, 1, 0), (10, 10, 1, -256)):
        assert q(*bad) == 0, bad
    assert inflate.DEFAULT_CHUNK_BYTES in (16384, 32768, 65536, 131072) and q(1, 1, 1, inflate.DEFAULT_CHUNK_BYTES)
    with pytest.raises(ValueError):
        inflate.DeviceInflater("cpu", chunk_bytes=1000)


def test_inflate_refusals_come_before_any_launch(lib):
    one, size = (C.c_long * 1)(5000), (C.c_long * 1)(20000)
    ws = lib.acimg_inflate_workspace(5000, 20000, 1, 1024)

    def call(src=A, lengths=one, sizes=size, count=1, chunk=1024, out=A, status=A, end=A, w=A, nws=ws):
        return lib.acimg_inflate(src, lengths, sizes, count, chunk, out, status, end, w, nws, None)

    for kw in (dict(src=None), dict(lengths=None), dict(sizes=None), dict(out=None), dict(status=None), dict(end=None),
               dict(w=None)):
        assert call(**kw) == EINVAL and "null" in _last_error(lib), kw
    assert call(count=0) == EINVAL and "count" in _last_error(lib)
    assert call(count=-2) == EINVAL
    assert call(lengths=(C.c_long * 1)(0)) == EINVAL and "0 bytes" in _last_error(lib)
    assert call(sizes=(C.c_long * 1)(0)) == EINVAL and "expected" in _last_error(lib)
    assert call(sizes=(C.c_long * 1)(2 ** 31)) == EINVAL and "expected" in _last_error(lib)
    assert call(lengths=(C.c_long * 2)(10, -1), sizes=(C.c_long * 2)(5, 5), count=2) == EINVAL and "stream 1" in _last_error(lib)
    for chunk in (0, 128, 1000, 1 << 25, -1024):
        assert call(chunk=chunk) == EINVAL and "chunk_bytes" in _last_error(lib), chunk
    assert call(w=A + 8) == EINVAL and "aligned" in _last_error(lib)
    assert call(nws=ws - 1) == EWORKSPACE and "workspace" in _last_error(lib)
    assert call(nws=0) == EWORKSPACE


# ---- 6 the loader's switch ----------------------------------------------------------------------------------------------------------
def test_loader_refuses_an_unknown_inflate():
    from acimg.data import DeviceDataLoader
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="inflate"):
            DeviceDataLoader(["a.tfrecord"], 4, inflate=bad)
