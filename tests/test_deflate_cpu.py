"""The device DEFLATE encoder without a GPU: the restatement (tests/deflate_ref.py - the device's parse rule, code
construction and header choices) against zlib's own decoder on every payload of tests/deflate_cases.py; the containers of
acimg.deflate against `gzip` / `zlib`; the code construction's properties on synthetic histograms; the refusals of the C
entry points with fake pointers (a call that fails to refuse reaches a launch and comes back as ACIMG_ELAUNCH here); and the
default (zlib) paths of `write_tfrecord` / `encode_png`, which must write what they always wrote.  A census of the
payloads (tests/deflate_census.py) holds them to the paths of `deflate_block_kernel` they are there to reach."""
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
import deflate_census as census  # noqa: E402
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


@pytest.mark.parametrize("name,payloads", cases.many_block_calls(), ids=[n for n, _ in cases.many_block_calls()])
def test_many_block_calls_inflate_and_cross_the_offsets_threads(name, payloads):
    """the expected streams of the GPU test's two calls, without a GPU; and the calls are what they are meant to be"""
    nblocks, per_thread, runs = cases.block_runs(payloads)
    memo = {}
    for p in payloads:
        if p not in memo:
            memo[p] = ref.deflate(p)
            assert zlib.decompress(memo[p], -15) == p and len(memo[p]) <= ref.bound(len(p))
    across = [r for r in runs if r[0] // per_thread != r[1] // per_thread]
    if name == "1025_of_one_byte":
        assert (nblocks, per_thread, across) == (1025, 2, []) and all(len(p) == 1 for p in payloads)
        assert all(a != b for a, b in zip(payloads, payloads[1:]))
    else:
        assert nblocks >= 2049 and per_thread >= 3
        assert sorted(len(p) for p in payloads if len(p) > 3) == [cases.B + 1, 2 * cases.B, 3 * cases.B + 17]
        assert len(across) == 3 and runs[-1] in across                    # the last payload's `first` is another thread's block


# ---- 1b what the payloads reach ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counted():
    """name -> [census.Block]; computed once, shared"""
    return {name: census.census_blocks(p) for name, p in cases.PAYLOADS}


ROWS = (("widest token, bits", "widest"), ("tokens wider than 32 bits", "over_32"),
        ("tokens that reach a third word", "third_word"), ("the largest shift of one of those", "third_word_shift"),
        ("length codes emitted", "length_codes"), ("match lengths emitted", "lengths"),
        ("distance codes emitted", "dist_codes"), ("largest distance", "dist_max"),
        ("longest code: literal/length, distance, code-length", "longest"),
        ("blocks where the limiter acts: the same three", "limited"), ("HCLEN sent (count of lengths)", "hclen"),
        ("pad bits before a marker", "pads"), ("bytes off the stored-or-dynamic edge", "off_the_edge"),
        ("matches cut by the block's end", "clipped"), ("the one used distance code of blocks with one", "one_dist_code"))


def _short(v):
    return "%d of them" % len(v) if isinstance(v, list) and len(v) > 12 else v


def test_the_payloads_reach_every_listed_feature(counted):
    """every path of `deflate_block_kernel` that DESIGN section 8 lists is taken by a payload of PAYLOADS; each condition names
    the payload that provides it, so taking a payload away, or a change of the parse rule that defuses one, fails here"""
    B = ref.BLOCK
    mild = census.table([b for name, _ in cases.MILD for b in counted[name]])
    total = census.table([b for blocks in counted.values() for b in blocks])
    print("\n%d blocks (%d dynamic, %d stored) -> %d (%d, %d)" % (mild["blocks"], mild["dynamic"], mild["stored"], total["blocks"],
                                                                 total["dynamic"], total["stored"]))
    for title, key in ROWS:
        print("%-56s %s -> %s" % (title, _short(mild[key]), _short(total[key])))

    # every_length: every match length, so every length code with every value of its extra bits; 257 and 258 in one block
    blocks = counted["every_length"]
    assert all(b.dynamic for b in blocks) and len(blocks) == 3
    assert set().union(*[b.lengths for b in blocks]) == set(range(3, 259))
    assert set().union(*[b.length_codes for b in blocks]) == set(range(29))
    assert {257, 258} <= blocks[0].lengths                                 # symbol 284 with extra 30 against symbol 285

    # every_distance_code.  A match has three bytes, so the largest distance a block of B bytes can hold is B - 3 (the copy at
    # B - 3, the source at 0), not B - 1: that one stands for "the largest" of code 27 and of the block
    first, last = counted["every_distance_code"]
    assert cases.LARGEST_DISTANCE == B - 3 and first.dynamic and last.dynamic
    wanted = cases.edge_distances()
    assert wanted[:4] == [1, 2, 3, 4] and wanted[-2:] == [12289, B - 3] and len(wanted) == 4 + 2 * 24
    assert all(ref.dist_code(d)[0] + 1 == ref.dist_code(d + 1)[0] for d in wanted[5:-1:2])      # each the last of its code
    assert all(ref.dist_code(d)[0] - 1 == ref.dist_code(d - 1)[0] for d in wanted[4::2])        # each the first of its code
    assert set(wanted) <= first.dists and first.dist_codes == set(range(28)) and first.dist_max == B - 3
    assert [p % ref.CHUNK for p, l, d in first.plan.toks if l and d == 2] == [0]
    assert total["dist_codes"] == list(range(28)) and 1 not in mild["dist_codes"]
    # matches cut by min(258, n - p): the one that ends a block of exactly B bytes, the one that ends a short last block
    assert first.n == B and not first.final and first.clipped == [(B - 3, 3, B - 3)]
    assert last.n == 700 and last.final and last.clipped == [(600, 100, 300)]
    assert counted["period4"][0].clipped == [(B - 132, 132, 128)]         # one of those that were there by chance

    # wide_tokens: 34 bits is the least that can reach a third word, the shift being 31 at most
    (wide,) = counted["wide_tokens"]
    assert wide.dynamic and wide.longest[:2] == (13, 10)
    far = [i for i, t in enumerate(wide.plan.toks) if t[1:] in cases.WIDE_FAR]
    assert len(far) == 4 and sorted(wide.widths[i] for i in far) == [39, 40, 40, 40]
    assert total["widest"] == 40 and mild["widest"] < 32
    assert len(wide.third_word) == 2 and set(wide.third_word) <= set(far)
    assert all(wide.shifts[i] >= 27 and wide.shifts[i] + wide.widths[i] > 64 for i in wide.third_word)
    assert mild["over_32"] == mild["third_word"] == 0

    # pad bits: all of 0..7, and 2 and 3, the two sides of the marker rule, in consecutive blocks of one payload
    assert total["pads"] == list(range(8)) and 2 not in mild["pads"]
    blocks = counted["pad_bits_2_then_3"]
    assert [(b.pad, b.dynamic, b.final) for b in blocks[:2]] == [(2, True, False), (3, True, False)]
    payload = dict(cases.PAYLOADS)["pad_bits_2_then_3"]
    coded = [ref.code_block(payload[s:s + B], False) for s in (0, B)]
    assert coded[0].endswith(ref.SYNC) and len(coded[0]) == blocks[0].plan.dyn_bytes + 5
    assert coded[1].endswith(ref.SYNC[1:]) and len(coded[1]) == blocks[1].plan.dyn_bytes + 4

    # the stored-or-dynamic decision at its edge, both blocks non-final so that their markers are checked too
    blocks = counted["stored_or_dynamic_edge"]
    assert [(b.margin, b.dynamic, b.final, b.n) for b in blocks[:2]] == [(0, False, False, B), (-1, True, False, B)]
    assert mild["off_the_edge"] > 20 and total["off_the_edge"] == 0

    # HCLEN.  Every code length is sent as its own symbol and 16, 17, 18 never are, so HCLEN is one more than the last place
    # in CL_ORDER of a length in use.  A distance code with two or more lengths is complete, and over the 28 distance
    # symbols a block can use a complete code has a length of 4 or less (28 * 2^-5 < 1); one used distance gets length 1.
    # Of 1..4 it is 4 that stands first in CL_ORDER, at place 11, behind 0 and 5..11: HCLEN 12 is the smallest there is.
    assert min(ref.CL_ORDER.index(l) for l in (1, 2, 3, 4)) + 1 == 12 and set(ref.CL_ORDER[3:12]) == {0} | set(range(4, 12))
    (small,) = counted["smallest_hclen"]
    assert small.dynamic and small.hclen == 12 == total["hclen"][0] and mild["hclen"][0] == 14
    assert counted["zeros_%d" % B][0].hclen == 18                          # the largest below 19: a code of 1 bit in use

    # a block with one used distance code that is not symbol 0: the code of length 1 with HDIST > 1
    (one,) = counted["one_distance_code"]
    assert one.dynamic and one.used_dist_codes == [16] and one.hdist == 17 and one.plan.len_d[16] == 1
    assert set(mild["one_dist_code"]) == {0} and counted["zeros_%d" % B][0].used_dist_codes == [0]

    # a literal/length code of 15 bits inside the block kernel: once from a depth of exactly 15, once from the limiter
    (deep,) = counted["literal_code_depth_15"]
    assert deep.dynamic and deep.depth[0] == 15 == deep.longest[0] and not deep.limited[0] and deep.hclen == 19
    (limited,) = counted["literal_code_limited"]
    assert limited.dynamic and limited.depth[0] == 16 and limited.longest[0] == 15 and limited.limited[0] and limited.hclen == 19
    assert cases.check_lengths(limited.plan.hist_ll, limited.plan.len_ll, 15, "literal_code_limited") == 16
    assert mild["longest"] == (13, 12, 7) and mild["limited"][:2] == (0, 0) and 19 not in mild["hclen"]
    # the 17 710-byte Fibonacci payload is two blocks full of matches: its codes stay short and no limiter acts on it
    fib = counted["fibonacci_counts"]
    assert [b.longest[0] for b in fib] == [12, 9] and not any(any(b.limited) for b in fib)
    # the 7-bit limiter of the code-length alphabet is what the mild payloads do reach at 1024 threads
    assert mild["limited"][2] == 6 and any(b.limited[2] for b in counted["smooth_fixture"])


def test_planted_copies_are_taken_as_planted():
    """the Planter's claim: what it lists as placed is in the parse, token for token"""
    pl = cases.Planter(np.random.RandomState(31), 6000)
    for at, length, dist in ((300, 3, 1), (512, 3, 2), (800, 40, 300), (1500, 258, 1000), (5000, 7, 4097), (5997, 3, 5000)):
        pl.place(at, length, dist=dist, step=ref.CHUNK if dist < ref.CHUNK else 1)
    assert [d for _, _, d in pl.planted] == [1, 2, 300, 1000, 4097, 5000]
    assert set(pl.planted) <= set(ref.greedy_parse(np.frombuffer(pl.bytes(), np.uint8)))


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
