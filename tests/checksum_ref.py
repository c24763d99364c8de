"""What the checksum tests measure against, written independently of csrc/checksum.hip: the algebra that lets a CRC or an
Adler-32 be computed in pieces, in NumPy / plain Python, held against `zlib.crc32`, `zlib.adler32` and `acimg_crc32c` by
tests/test_checksum_cpu.py.

A 32-bit value stands for a polynomial over GF(2) in the standards' reflected order: bit 31 is x^0, bit 0 is x^31.
Without its init and its final XOR a CRC is linear:  pure(D) = D(x) x^32 mod P,
    pure(A || B) = pure(A) x^(8 |B|) ^ pure(B),     crc(D) = pure(D) ^ 0xFFFFFFFF x^(8 |D|) ^ 0xFFFFFFFF.
`crc_by_windows` restates the plan of the kernel: absolute 16384-byte windows with zeros outside the payload, zeros behind
the payload's last byte undone by a power of x^-1 = (P + 1) / x."""
import ctypes
import zlib

import numpy as np

POLY = {"crc32": 0xEDB88320, "crc32c": 0x82F63B78}
ONE, X = 0x80000000, 0x40000000
ADLER = 65521
MASK_DELTA = 0xa282ead8
SEGMENT, RUN = 16384, 64
KNOWN = b"123456789"
KNOWN_VALUES = {"crc32": 0xCBF43926, "crc32c": 0xE3069283, "adler32": 0x091E01DE}


def longs(*values):
    """a C array of long: the host tables of the C ABI"""
    return (ctypes.c_long * len(values))(*[int(v) for v in values])


def mulx(v, poly):
    """v x mod P"""
    return (v >> 1) ^ (poly if v & 1 else 0)


def gf_mul(a, b, poly):
    """a b mod P"""
    r = 0
    for i in range(32):
        if a & (ONE >> i):
            r ^= b
        b = mulx(b, poly)
    return r


def gf_pow(base, e, poly):
    r = ONE
    while e:
        if e & 1:
            r = gf_mul(r, base, poly)
        base = gf_mul(base, base, poly)
        e >>= 1
    return r


def xpow(e, poly):
    """x^e mod P"""
    return gf_pow(X, e, poly)


def xinv(poly):
    """x^-1 mod P: P has the constant term 1, so 1 = P + x Q and Q = (P + 1) / x"""
    return ((poly << 1) | 1) & 0xFFFFFFFF


def byte_table(poly):
    t = np.zeros(256, np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = mulx(c, poly)
        t[i] = c
    return t


_TABLES = {}


def pure(data, poly):
    """D(x) x^32 mod P, byte by byte: the CRC register started at 0, no final XOR"""
    if poly not in _TABLES:
        _TABLES[poly] = [int(v) for v in byte_table(poly)]
    t, c = _TABLES[poly], 0
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c


def init_term(n, poly):
    return gf_mul(0xFFFFFFFF, xpow(8 * n, poly), poly)


def finish(pure_value, n, poly):
    """the standard's CRC of n bytes from their pure value"""
    return pure_value ^ init_term(n, poly) ^ 0xFFFFFFFF


def combine(pure_a, pure_b, len_b, poly):
    """pure(A || B)"""
    return gf_mul(pure_a, xpow(8 * len_b, poly), poly) ^ pure_b


def crc(data, poly):
    return finish(pure(data, poly), len(data), poly)


def crc_in_pieces(data, cuts, poly):
    """the CRC of `data` from the pure values of its pieces between the sorted offsets `cuts`"""
    edges = [0] + list(cuts) + [len(data)]
    acc = 0
    for lo, hi in zip(edges[:-1], edges[1:]):
        acc = combine(acc, pure(data[lo:hi], poly), hi - lo, poly)
    return finish(acc, len(data), poly)


def mask(crc_value):
    return (((crc_value >> 15) | (crc_value << 17)) + MASK_DELTA) & 0xFFFFFFFF


def crc_by_windows(data, address, poly):
    """the CRC of `data` lying at byte address `address`, by the kernel's plan: every absolute SEGMENT window the payload
    touches is taken whole with zeros outside the payload; a window's value is multiplied by x^(8 behind) x^(-8 z), z the
    zeros behind the payload's last byte in it.  The values XOR together in any order."""
    data = bytes(data)
    a0, a1 = address, address + len(data)
    acc, w = 0, a0 - a0 % SEGMENT
    while w < a1:
        lo, hi = max(a0, w) - w, min(a1, w + SEGMENT) - w
        window = bytes(lo) + data[w + lo - a0:w + hi - a0] + bytes(SEGMENT - hi)
        behind = a1 - (w + hi)
        mult = gf_mul(xpow(8 * behind, poly), gf_pow(xinv(poly), 8 * (SEGMENT - hi), poly), poly)
        acc ^= gf_mul(pure(window, poly), mult, poly)
        w += SEGMENT
    return finish(acc, len(data), poly)


def window_by_lanes(window, poly):
    """pure(window) of one SEGMENT window by the kernel's lanes: lane t folds its RUN bytes as four 16-byte words in Horner
    form over little-endian dwords, c = (c ^ d0) x^128 ^ d1 x^96 ^ d2 x^64 ^ d3 x^32; a butterfly over 64 lanes multiplies
    the lower value of a pair by x^(bits of the upper block); four waves combine with x^(bits of the waves behind)"""
    d = np.frombuffer(bytes(window), "<u4").reshape(SEGMENT // RUN, RUN // 16, 4)
    k = {e: xpow(e, poly) for e in (128, 96, 64, 32)}
    lanes = []
    for t in range(SEGMENT // RUN):
        c = 0
        for j in range(RUN // 16):
            w = [int(v) for v in d[t, j]]
            c = gf_mul(c ^ w[0], k[128], poly) ^ gf_mul(w[1], k[96], poly) ^ gf_mul(w[2], k[64], poly) ^ gf_mul(w[3], k[32], poly)
        lanes.append(c)
    waves = []
    for w0 in range(0, len(lanes), 64):
        v = lanes[w0:w0 + 64]
        for level in range(6):
            off, m = 1 << level, xpow(8 * RUN << level, poly)
            v = [gf_mul(v[i & ~off], m, poly) ^ v[i | off] for i in range(64)]
        assert len(set(v)) == 1
        waves.append(v[0])
    wave_bits = 8 * 64 * RUN
    acc = 0
    for i, v in enumerate(waves):
        acc ^= gf_mul(v, xpow(wave_bits * (len(waves) - 1 - i), poly), poly)
    return acc


# ---- Adler-32 -------------------------------------------------------------------------------------------------------------
def adler_sums(data):
    """(sum b, sum (n - i) b) of a piece, exact (Python ints)"""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = d.size
    return int(d.sum()), int((d * (n - np.arange(n, dtype=np.int64))).sum())


def adler_in_pieces(data, cuts):
    """Adler-32 from the pieces' sums: A = 1 + sum A_s, B = n + sum (B_s + behind_s A_s), mod 65521"""
    edges = [0] + list(cuts) + [len(data)]
    a, b = 1, len(data)
    for lo, hi in zip(edges[:-1], edges[1:]):
        sa, sb = adler_sums(data[lo:hi])
        a += sa
        b += sb + (len(data) - hi) * sa
    return (b % ADLER) << 16 | (a % ADLER)


# ---- the oracles and the cases of the GPU test ---------------------------------------------------------------------------
def oracle(kind, data):
    """kind 0..3 of include/acimg.h by the host oracles: zlib.crc32, acimg_crc32c (masked for 2), zlib.adler32"""
    from acimg import tfio
    data = bytes(data)
    if kind == 0:
        return zlib.crc32(data) & 0xFFFFFFFF
    if kind == 3:
        return zlib.adler32(data) & 0xFFFFFFFF
    c = tfio.crc32c(data)
    return tfio.mask_crc(c) if kind == 2 else c


LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, RUN - 1, RUN, RUN + 1, 64 * RUN - 1, 64 * RUN, 64 * RUN + 1, SEGMENT - 1, SEGMENT,
           SEGMENT + 1, 2 * SEGMENT + 3]
SWEEP = 3 * 1024 * 1024 + 77          # larger than one sweep of a grid of 160 workgroups


def payload_set(seed=5):
    """[(name, bytes)]: every length of LENGTHS as random bytes, zeros and 0xFF (zeros pin the init term), empty payloads
    between non-empty ones, the Adler-32 overflow cases and one payload past a grid sweep"""
    rng = np.random.RandomState(seed)
    out = []
    for n in LENGTHS:
        out.append(("random_%d" % n, rng.randint(0, 256, n).astype(np.uint8).tobytes()))
        out.append(("zeros_%d" % n, bytes(n)))
        out.append(("ones_%d" % n, b"\xff" * n))
    out.append(("ff_5552", b"\xff" * 5552))
    out.append(("empty_between", b""))
    out.append(("ff_5553", b"\xff" * 5553))
    out.append(("ff_1MiB_1", b"\xff" * (1024 * 1024 + 1)))
    out.append(("01_65521", b"\x01" * 65521))
    out.append(("known", KNOWN))
    out.append(("sweep", rng.randint(0, 256, SWEEP).astype(np.uint8).tobytes()))
    out.append(("empty_last", b""))
    return out
