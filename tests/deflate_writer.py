"""A token-level DEFLATE writer for the tests: data in, bytes out.  It does no matching and builds no Huffman code - the
caller states every token, every code length and the code-length code, so a stream can hold what zlib's encoder never
writes (RFC 1951 allows all of it, and zlib's decoder reads it): 15-bit codes, all 19 code-length lengths, length 258 as
symbol 284 with extra 31, distance 32768, a repeat run that begins in the literal/length lengths and ends in the distance
lengths, stored blocks of any LEN at any bit phase.  Independent of tests/inflate_ref.py: its own tables, and `Stream`
expands the tokens itself, so the payload a stream was written for is known without any decoder."""

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in range(2))
RUN = {16: (3, 2), 17: (3, 3), 18: (11, 7)}          # repeat symbol -> (shortest run, extra bits)
FIXED_LL = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8
FIXED_D = (5,) * 32


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


def length_symbol(length, split_258=False):
    """-> (symbol, extra bits, extra value); split_258: 258 as symbol 284 with all five extra bits set"""
    if length == 258:
        return (284, 5, 31) if split_258 else (285, 0, 0)
    c = max(i for i in range(28) if LENGTH_BASE[i] <= length)
    assert length - LENGTH_BASE[c] < 1 << LENGTH_EXTRA[c]
    return 257 + c, LENGTH_EXTRA[c], length - LENGTH_BASE[c]


def dist_symbol(dist):
    c = max(i for i in range(30) if DIST_BASE[i] <= dist)
    assert dist - DIST_BASE[c] < 1 << DIST_EXTRA[c]
    return c, DIST_EXTRA[c], dist - DIST_BASE[c]


def lens_of(size, assigned):
    """{symbol: length} -> the list of `size` code lengths"""
    assert max(assigned) < size
    return [assigned.get(s, 0) for s in range(size)]


class Stream(object):
    """blocks appended to one BitWriter, and the bytes they inflate to.  A token is a literal byte or (length, distance)."""

    def __init__(self):
        self.w, self.out = BitWriter(), bytearray()

    def expand(self, tokens):
        for t in tokens:
            if isinstance(t, int):
                self.out.append(t)
            else:
                length, dist = t
                assert 3 <= length <= 258 and 1 <= dist <= min(32768, len(self.out)), t
                for _ in range(length):
                    self.out.append(self.out[-dist])

    def stored(self, data, final=0):
        assert len(data) <= 65535
        self.w.bits(final, 1).bits(0, 2).align().bits(len(data), 16).bits(~len(data), 16).raw(data)
        self.out += data
        return self

    def _tokens(self, tokens, ll, d, split_258, eob):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*ll[t])
                continue
            s, k, x = length_symbol(t[0], split_258)
            w.code(*ll[s]).bits(x, k)
            s, k, x = dist_symbol(t[1])
            w.code(*d[s]).bits(x, k)
        if eob:
            w.code(*ll[256])
        self.expand(tokens)
        return self

    def fixed(self, tokens, final=0, split_258=False, eob=True):
        self.w.bits(final, 1).bits(1, 2)
        return self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), split_258, eob)

    def dynamic(self, tokens, ll_lens, d_lens, cl_lens, final=0, split_258=False, runs=(), eob=True):
        """ll_lens: 257..286 literal/length code lengths (HLIT follows from their number), d_lens: 1..30 distance code lengths,
        cl_lens: the 19 lengths of the code-length code by symbol.  Every length is written as itself except the stretches
        `runs` names: (start, stop, symbol) writes positions start..stop-1 of the joined sequence as ONE repeat-16/17/18
        run, across the boundary of the two alphabets or past the end if the caller says so."""
        w = self.w
        lens = list(ll_lens) + list(d_lens)
        assert 257 <= len(ll_lens) <= 286 and 1 <= len(d_lens) <= 30 and len(cl_lens) == 19
        hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1)
        w.bits(final, 1).bits(2, 2).bits(len(ll_lens) - 257, 5).bits(len(d_lens) - 1, 5).bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)
        run_at = {start: (stop, s) for start, stop, s in runs}
        i = 0
        while i < len(lens):
            if i in run_at:
                stop, s = run_at[i]
                value = lens[i - 1] if s == 16 else 0
                assert 0 <= stop - i - RUN[s][0] < 1 << RUN[s][1] and all(l == value for l in lens[i:stop]), (i, stop, s)
                w.code(*cl[s]).bits(stop - i - RUN[s][0], RUN[s][1])
                i = stop
            else:
                w.code(*cl[lens[i]])
                i += 1
        return self._tokens(tokens, canonical(ll_lens), canonical(d_lens), split_258, eob)

    def bytes(self):
        return self.w.bytes()
