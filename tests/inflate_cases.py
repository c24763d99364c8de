"""The streams that tests/test_inflate_cpu.py runs through the restatement (tests/inflate_ref.py) and
tests/test_inflate_gpu.py through the device: (name, raw deflate stream, payload), built once per process, never modified.
Payloads are small because the restatement is slow; small blocks come from memLevel 1 (128-symbol blocks) and small
`chunk_bytes`, not from large inputs.  Every stream is checked against zlib when the module is imported."""
import zlib

import numpy as np

import deflate_ref
import inflate_ref

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
class BitWriter(object):
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        return self

    def code(self, code, length):
        """a Huffman code, most significant bit first"""
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def raw(self, data):
        self.align()
        for b in data:
            self.bits(b, 8)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def canonical(lens):
    """symbol -> (code, length) of the canonical code of `lens` (RFC 1951 3.2.2)"""
    out, code = {}, 0
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                out[s] = (code, L)
                code += 1
        code <<= 1
    return out


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
    for name, stream, payload in out:
        assert zlib.decompress(stream, -15) == payload, name
    return out


CASES = _cases()
COVERAGE_CASE = "smooth64k-mem1"
