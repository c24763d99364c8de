"""The streams that tests/test_inflate_cpu.py runs through the restatement (tests/inflate_ref.py) and
tests/test_inflate_gpu.py through the device: (name, raw deflate stream, payload), built once per process, never modified.
Payloads are small because the restatement is slow; small blocks come from memLevel 1 (128-symbol blocks) and small
`chunk_bytes`, not from large inputs.  What zlib's encoder never writes - 15-bit codes, all 19 code-length lengths, distance
32768, repeat runs across the two alphabets, stored blocks at every bit phase - comes from the token-level writer
(tests/deflate_writer.py); tests/inflate_census.py counts what the streams reach.  Every stream is checked against zlib when
the module is imported."""
import zlib

import numpy as np

import deflate_ref
import inflate_ref
from deflate_writer import CL_ORDER, BitWriter, Stream, canonical, lens_of  # noqa: F401

CHUNKS = (256, 1024, 4096, 1 << 22)          # the last: the whole stream in one chunk
GPU_CHUNK = 1024                             # what the GPU test decodes every case with


def smooth_ramp(rows, cols=512):
    y, x = np.mgrid[0:rows, 0:cols]
    return ((y * 3 + x // 2 + 20 * np.sin(x / 37.0) + 9 * np.cos(y / 11.0)) % 256).astype(np.uint8)


def _inflate_payloads():
    rng = np.random.RandomState(11)
    n = 12288
    smooth = smooth_ramp(n // 512).tobytes()
    noisy = (smooth_ramp(n // 512) + rng.randint(0, 4, (n // 512, 512))).astype(np.uint8).tobytes()
    t = np.arange(n // 4)
    tone = (2 ** 22 * np.sin(2 * np.pi * 700.0 * t / 12288.0) + rng.randn(t.size) * 2 ** 12).astype("<i4").tobytes()
    return [("one_byte", b"\x5a"), ("zeros", bytes(n)), ("period3", (b"\x01\x7f\xfe" * n)[:n]), ("smooth", smooth),
            ("smooth_noise", noisy), ("random", rng.randint(0, 256, n).astype(np.uint8).tobytes()), ("tone_int32", tone)]


def _compress(payload, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if flush is None:
        return co.compress(payload) + co.flush()
    half = len(payload) // 2
    return co.compress(payload[:half]) + co.flush(flush) + co.compress(payload[half:]) + co.flush()


COMPRESSIONS = (("level0", dict(level=0)), ("level1", dict(level=1)), ("level6", dict(level=6)), ("level9", dict(level=9)),
                ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                ("rle", dict(strategy=zlib.Z_RLE)), ("mem1", dict(mem=1)), ("mem1_level9", dict(mem=1, level=9)),
                ("sync_flush", dict(mem=1, flush=zlib.Z_SYNC_FLUSH)), ("full_flush", dict(flush=zlib.Z_FULL_FLUSH)))


# ---- hand-made streams -----------------------------------------------------------------------------------------------------------
def dynamic_block(w, final=1, btype=2, hlit=0, hdist=0, cl_lens=None, seq=None, body=((0, 1), (0, 1), (0, 1), (1, 1))):
    """one hand-made dynamic block into the BitWriter `w`.  The defaults are the valid block of b"aaa": literal 97 and the
    end-of-block symbol have length 1, one distance length of 0; the code-length code knows 18 (1 bit), 0 and 1 (2 bits).
    seq: the code-length symbols as (symbol, extra value); body: the (code, length) pairs after the header."""
    if cl_lens is None:
        cl_lens = {18: 1, 0: 2, 1: 2}
    if seq is None:
        seq = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (1, 0), (0, 0)]
    lens = [cl_lens.get(s, 0) for s in range(19)]
    hclen = max(i for i, s in enumerate(CL_ORDER) if lens[s]) + 1
    hclen = max(hclen, 4)
    w.bits(final, 1).bits(btype, 2).bits(hlit, 5).bits(hdist, 5).bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(lens[s], 3)
    codes = canonical(lens)
    extra = {16: 2, 17: 3, 18: 7}
    for s, x in seq:
        w.code(*codes[s])
        if s in extra:
            w.bits(x, extra[s])
    for c, l in body:
        w.code(c, l)
    return w


def single_length_one_code():
    """a non-final dynamic block whose literal/length code is ONE code of length 1 (the end-of-block symbol; incomplete, and
    zlib accepts exactly this), then a final stored block"""
    w = BitWriter()
    dynamic_block(w, final=0, seq=[(18, 138 - 11), (18, 118 - 11), (1, 0), (0, 0)], body=((0, 1),))
    w.bits(1, 1).bits(0, 2).align().bits(5, 16).bits(~5, 16).raw(b"hello")
    return w.bytes(), b"hello"


def false_start(chunk_bytes=GPU_CHUNK):
    """a stored stream (level 0) of random bytes with the first bytes of a real dynamic block spliced into the payload so
    that they begin exactly at chunk 1's lowest offset: the finder must take them, the chain must not"""
    rng = np.random.RandomState(23)
    payload = bytearray(rng.randint(0, 256, 3 * chunk_bytes).astype(np.uint8).tobytes())
    image = smooth_ramp(24).tobytes()
    donor = _compress(image, mem=1)
    at = [bit for bit, final, btype in inflate_ref.block_headers(donor, len(image)) if not final and btype == 2][0]
    bait = ((int.from_bytes(donor, "little") >> at) & ((1 << 2400) - 1)).to_bytes(300, "little")      # from that header on
    assert bait[0] & 7 == 4 and inflate_ref.is_start(bait, 0)
    payload[chunk_bytes - 5:chunk_bytes - 5 + len(bait)] = bait        # the stored block's header is 5 bytes
    payload = bytes(payload)
    stream = _compress(payload, level=0)
    assert stream[chunk_bytes:chunk_bytes + len(bait)] == bait
    return stream, payload


def window_spanning():
    """2000 random bytes, 30000 compressible ones, the 2000 again: with level 9 the second copy is coded as matches about
    32000 back, and with memLevel 1 a 256-byte chunk inflates to far less than the window - a marker's source lies many
    live chunks back"""
    rng = np.random.RandomState(31)
    a = rng.randint(0, 256, 2000).astype(np.uint8).tobytes()
    mid = (smooth_ramp(60)[:, :500] // 8 * 8 + rng.randint(0, 2, (60, 500))).astype(np.uint8).tobytes()
    payload = a + mid + a
    return _compress(payload, level=9, mem=1), payload


# ---- token-level streams (tests/deflate_writer.py): what RFC 1951 allows and zlib's encoder never writes ------------------------
# two complete code-length codes over all 19 symbols, so HCLEN is 15 and symbol 15 (last in the header's order) has a code:
# 13 four-bit and 6 five-bit codes; 15 four-bit codes, one of 5 and of 6 bits and two of 7 bits (lengths 12 and 13)
CL_ALL = [5 if s in (10, 11, 12, 13, 14, 16) else 4 for s in range(19)]
CL_DEEP = [{10: 5, 11: 6, 12: 7, 13: 7}.get(s, 4) for s in range(19)]


def flat(symbols):
    """{symbol: length} of a complete code of two neighbouring lengths"""
    n = len(symbols)
    k = n.bit_length() - 1
    return {s: k if i < (2 << k) - n else k + 1 for i, s in enumerate(symbols)}


def chain(symbols):
    """{symbol: length} of the complete code of lengths 1, 2, .. 14, 15, 15 over 16 symbols"""
    assert len(symbols) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


def _random(seed, n):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


DEEP_LL = lens_of(286, chain([97, 98, 99, 100, 101, 102, 103, 104, 257, 264, 105, 285, 256, 121, 122, 284]))
DEEP_D = lens_of(30, chain([0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22]))
DEEP_RUNS = ((0, 97, 18), (123, 133, 17), (134, 140, 16))        # zero lengths, so the code-length symbols 16..18 are decoded too


def deep_block(s, k, final=0):
    """a dynamic block of 14- and 15-bit literals (y, z: 121, 122) and of copies through the distance codes of 15 bits (the
    first two, far before the block), 14, 13, 12, 11 and 10 bits; length 258 as 285 in even blocks, as 284 + 31 in odd ones"""
    tokens = [(3, 2049 + 7 * k), (10, 1025 + k), (3, 513 + k)] + [122, 121, 122, 97 + k % 8] * 30
    tokens += [(3, 300), (3, 150), (10, 70), (3, 40), (258, 1), (258, 2), 105, (258, 3)] + [122] * 20
    return s.dynamic(tokens, DEEP_LL, DEEP_D, CL_DEEP, final=final, split_258=bool(k & 1), runs=DEEP_RUNS)


def deep_codes():
    s = Stream().stored(_random(41, 3200))
    for k in range(6):
        deep_block(s, k)
    deep_block(s, 6, final=1)
    return s.bytes(), bytes(s.out)


def run_crosses_alphabets():
    """three blocks, each in a chunk of its own behind 1100 stored bytes: a repeat-16 run of length 3 over literal/length
    symbols 284, 285 and distance codes 0..2 (HLIT = HDIST = 29), a repeat-17 and a repeat-18 run of zeros over the end of
    the one alphabet and the start of the other.  The tokens use the codes on both sides of each run."""
    s = Stream().stored(_random(42, 1100))
    ll = lens_of(286, {sym: 3 for sym in (97, 98, 99, 100, 256, 283, 284, 285)})
    s.dynamic([97, 98, 99, 100, (258, 2), (230, 3), (200, 1), 97], ll, lens_of(30, {c: 3 for c in range(8)}), CL_ALL,
              runs=((284, 289, 16),))
    ll = lens_of(286, {sym: 3 for sym in (97, 98, 99, 100, 101, 102, 256, 257)})
    d = lens_of(8, {c: 2 for c in (4, 5, 6, 7)})
    for run in ((282, 290, 17), (258, 290, 18)):
        s.stored(_random(43 + run[2], 1100))
        s.dynamic([97, 98, 99, 100, 101, 102, (3, 5), (3, 8), (3, 9), (3, 16), 97], ll, d, CL_ALL, runs=(run,))
    s.stored(b"tail", final=1)
    return s.bytes(), bytes(s.out)


def far_and_long():
    """32768 stored bytes; two fixed blocks (not sought by the finder: chunk 0 decodes them) that begin with distance 32768 at
    exactly 32768 bytes and copy 258 bytes at distances 1, 2, 63, 64, 65 and 257, 258 as symbol 285 and as 284 + 31; the
    same in two dynamic blocks that later chunks decode, each with distance 32768 into the stored bytes"""
    s = Stream().stored(_random(44, 32768))
    near = [(258, d) for d in (1, 2, 63, 64, 65, 257)]
    s.fixed([(3, 32768)] + near + [(258, 32768)])
    s.fixed(near + [(4, 32768)], split_258=True)
    ll = lens_of(286, flat([97, 98, 99, 100, 256, 257, 284, 285]))
    d = lens_of(30, flat([0, 1, 11, 12, 16, 29]))
    for split in (False, True):
        s.dynamic([97, 98, 99, 100] * 80 + near + [(3, 32768), (258, 32768), (250, 32768)], ll, d, CL_ALL, split_258=split)
    s.fixed([33], final=1)
    return s.bytes(), bytes(s.out)


def copy_straddles_chunk_start():
    """two dynamic blocks, each the start of a chunk at chunk_bytes 256 and 1024, whose first copy begins before the chunk's
    first byte and runs into the chunk's own: 10 bytes from 12 back after 5 literals; 100 bytes from 7 back after 3"""
    s = Stream().stored(_random(45, 2000))
    ll = lens_of(280, flat([97, 98, 99, 100, 256, 264, 279]))
    d = lens_of(7, flat([5, 6]))
    s.dynamic([97, 98, 99, 100, 97, (10, 12)] + [98, 99] * 30, ll, d, CL_ALL)
    s.stored(_random(46, 1100))
    s.dynamic([97, 98, 99, (100, 7)] + [100, 97] * 30 + [(10, 11)], ll, d, CL_ALL)
    s.stored(b"end", final=1)
    return s.bytes(), bytes(s.out)


LITERAL_RUNS = (63, 64, 65, 128, 129)


def literal_runs():
    """per N: N literals and a copy; N literals, the end of the block and a stored block; N literals, the end of the block
    and a block that begins with a copy.  Every run begins right behind a copy.  The stream ends in a run of 63."""
    s = Stream().stored(b"0123456789abcdef")
    ll = lens_of(259, flat([97, 98, 99, 100, 256, 257, 258]))
    d = lens_of(2, flat([0, 1]))
    for n in LITERAL_RUNS:
        lits = [97 + i % 4 for i in range(n)]
        s.dynamic([(3, 1)] + lits + [(4, 2)] + lits, ll, d, CL_ALL)
        s.stored(b"--stored")
        s.dynamic([(3, 1)] + lits, ll, d, CL_ALL)
        s.fixed([(3, 1), 65])
    s.dynamic([(3, 1)] + [97 + i % 4 for i in range(63)], ll, d, CL_ALL, final=1)
    return s.bytes(), bytes(s.out)


def stored_edges():
    """LEN 0 between two dynamic blocks; a stored header at each of the 8 bit phases (behind a fixed block of n nine-bit
    literals, 10 + 9 n bits); a stored block that ends on a multiple of 1024 bytes in front of a non-final dynamic block;
    a final fixed block of 64 bits from a byte boundary, so the stream's last bit is its last byte's last"""
    s = Stream()
    ll, d = lens_of(258, flat([97, 98, 256, 257])), lens_of(2, flat([0, 1]))
    s.dynamic([97, 98, (3, 1)], ll, d, CL_ALL).stored(b"").dynamic([98, (3, 2)], ll, d, CL_ALL)
    for phase in range(8):
        s.stored(b"|")
        assert s.w.n % 8 == 0
        s.fixed([200] * ((phase - 2) % 8))
        assert s.w.n % 8 == phase
        s.stored(b"phase %d" % phase)
    fill = -(s.w.n // 8 + 5) % 1024
    s.stored(_random(47, fill))
    assert s.w.n % (8 * 1024) == 0
    s.dynamic([97] * 40 + [(3, 1)], ll, d, CL_ALL)
    s.stored(b"q").fixed([200] * 6, final=1)
    assert s.w.n % 8 == 0
    return s.bytes(), bytes(s.out)


def stored_len_65535():
    """the largest stored block, three empty fixed blocks and a final fixed block of one nine-bit literal: 49 bits, so 7
    pad bits end the stream; 64 KiB of payload"""
    s = Stream().stored(smooth_ramp(128).tobytes()[:65535])
    s.fixed([]).fixed([]).fixed([]).fixed([200], final=1)
    assert s.w.n % 8 == 1 and len(s.out) == 65536
    return s.bytes(), bytes(s.out)


TOKEN_CASES = (("deep_codes", deep_codes), ("run_crosses_alphabets", run_crosses_alphabets), ("far_and_long", far_and_long),
               ("copy_straddles_chunk_start", copy_straddles_chunk_start), ("literal_runs", literal_runs),
               ("stored_edges", stored_edges), ("stored_edges-len_65535", stored_len_65535))
# the token-level streams that are decoded at every chunk size (tests/test_inflate_gpu.py: SMALL_CHUNK_CASES)
TOKEN_SMALL_CHUNK_CASES = tuple(name for name, _ in TOKEN_CASES[:6])


def token_corrupt_streams():
    """(name, stream, expected size): broken streams that need the token-level writer; zlib refuses every one"""
    out = []
    for sym in (286, 287):          # the fixed code has codes for them (8 bits, 0xC0 + symbol - 280); no block may use them
        w = BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 97, 8).code(0xC0 + sym - 280, 8)
        out.append(("fixed_literal_length_symbol_%d" % sym, w.bytes() + bytes(8), 4))
    for code in (30, 31):
        w = BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 97, 8).code(1, 7).code(code, 5)
        out.append(("fixed_distance_code_%d" % code, w.bytes() + bytes(8), 4))
    s = Stream()                    # a length symbol (257: code 11) where the only distance length is 0
    s.dynamic([97], lens_of(258, {97: 1, 256: 2, 257: 2}), [0], CL_ALL, final=1, eob=False)
    s.w.code(3, 2)
    out.append(("length_symbol_without_a_distance_code", s.bytes() + bytes(8), 4))
    s = Stream()                    # 286 + 4 lengths; a repeat-18 run of 33 zeros from 258 on ends one behind the last
    s.dynamic([97], lens_of(286, {sym: 3 for sym in (97, 98, 99, 100, 101, 102, 256, 257)}), [0, 0, 0, 0], CL_ALL, final=1,
              runs=((258, 291, 18),))
    out.append(("crossing_run_past_the_total", s.bytes() + bytes(8), 1))
    header = Stream().dynamic([], DEEP_LL, DEEP_D, CL_DEEP, final=1, runs=DEEP_RUNS, eob=False).w.n
    cut = Stream().dynamic([122] * 20, DEEP_LL, DEEP_D, CL_DEEP, final=1, runs=DEEP_RUNS).bytes()[:(header + 45) // 8 + 1]
    assert header + 45 < 8 * len(cut) < header + 60
    out.append(("cut_inside_a_15_bit_code", cut, 20))
    return out


# (name, arguments of dynamic_block that break ONE field of the valid hand-made block)
BROKEN_HEADERS = [
    ("btype_3", dict(btype=3)),
    ("hlit_30", dict(hlit=30)),
    ("hdist_30", dict(hdist=30)),
    ("code_length_code_over_subscribed", dict(cl_lens={18: 1, 0: 1, 1: 1})),
    ("code_length_code_incomplete", dict(cl_lens={18: 2, 0: 2, 1: 2})),
    ("repeat_16_first", dict(cl_lens={18: 1, 16: 2, 1: 3, 0: 3}, seq=[(16, 0)])),
    ("run_past_the_total", dict(seq=[(18, 138 - 11), (18, 138 - 11)])),
    ("no_end_of_block_code", dict(seq=[(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 21 - 11), (1, 0)])),
    ("literal_code_over_subscribed", dict(seq=[(18, 97 - 11), (1, 0), (1, 0), (18, 138 - 11), (18, 19 - 11), (1, 0), (0, 0)])),
    ("literal_code_incomplete", dict(cl_lens={18: 1, 0: 2, 2: 2},
                                      seq=[(18, 97 - 11), (2, 0), (18, 138 - 11), (18, 20 - 11), (2, 0), (0, 0)])),
    ("invalid_literal_code", dict(seq=[(18, 138 - 11), (18, 118 - 11), (1, 0), (0, 0)], body=((1, 1),))),
]


def corrupt_streams():
    """(name, stream, expected size, status): what the decoder must end with that status on"""
    by_name = {name: (stream, payload) for name, stream, payload in CASES}
    out = [(name, dynamic_block(BitWriter(), **kw).bytes() + bytes(8), 3, inflate_ref.CORRUPT) for name, kw in BROKEN_HEADERS]
    far = BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7).bytes()
    out.append(("distance_before_the_stream", far, 4, inflate_ref.CORRUPT))
    stored = BitWriter().bits(1, 1).bits(0, 2).align().bits(5, 16).bits(~5 ^ 1, 16).raw(b"hello").bytes()
    out.append(("len_nlen", stored, 5, inflate_ref.CORRUPT))
    stream, payload = by_name["smooth64k-mem1"]
    out.append(("truncated_in_a_later_chunk", stream[:9000], len(payload), inflate_ref.TRUNCATED))
    out.append(("one_byte_more_expected", stream, len(payload) + 1, inflate_ref.SIZE))
    out.append(("one_byte_less_expected", stream, len(payload) - 1, inflate_ref.SIZE))
    flipped = bytearray(stream)
    flipped[5003] ^= 0x10
    out.append(("a_flipped_bit_in_a_later_chunk", bytes(flipped), len(payload), inflate_ref.CORRUPT))
    for name, stream, size in token_corrupt_streams():
        out.append((name, stream, size, inflate_ref.inflate(stream, size, GPU_CHUNK).status))      # checked against zlib in the CPU test
    return out


def _cases():
    out = []
    for kind, payload in _inflate_payloads():
        for cname, kw in COMPRESSIONS:
            out.append(("%s-%s" % (kind, cname), _compress(payload, **kw), payload))
        out.append(("%s-device_encoder" % kind, deflate_ref.deflate(payload), payload))
    out.append(("smooth64k-mem1", _compress(smooth_ramp(128).tobytes(), mem=1), smooth_ramp(128).tobytes()))
    # the device encoder's 16 KiB blocks with their sync markers, one of them with a single distance code (a run of zeros)
    two = bytes(deflate_ref.BLOCK) + smooth_ramp(40).tobytes()
    out.append(("zeros_then_smooth-device_encoder", deflate_ref.deflate(two), two))
    out.append(("window_spanning",) + window_spanning())
    out.append(("single_length_one_code",) + single_length_one_code())
    out.append(("false_start",) + false_start())
    out.extend((name,) + make() for name, make in TOKEN_CASES)
    for name, stream, payload in out:
        assert zlib.decompress(stream, -15) == payload, name
    return out


CASES = _cases()
COVERAGE_CASE = "smooth64k-mem1"
