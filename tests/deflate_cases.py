"""The payloads and histograms that tests/test_deflate_cpu.py runs through the restatement and tests/test_deflate_gpu.py
through the device: built once per process, never modified."""
import os

import numpy as np

import deflate_ref as ref

B = ref.BLOCK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode_golden.npz")


def fibonacci(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def smooth_fixture():
    """the 196608 bytes of pixels_smooth_420_256x256 of the committed JPEG fixture"""
    with np.load(GOLDEN) as g:
        return g["pixels_smooth_420_256x256"].tobytes()


def _payloads():
    rng = np.random.RandomState(5)
    noise = rng.randint(0, 256, 3 * B + 17).astype(np.uint8).tobytes()
    out = []
    for n in (1, 2, 3, B - 1, B, B + 1, 3 * B + 17):                      # B + 1: a one-byte last block
        out.append(("zeros_%d" % n, bytes(n)))                           # runs of 258 at distance 1
        out.append(("noise_%d" % n, noise[:n]))                          # the stored fallback
    out.append(("period3", (b"\x01\x7f\xfe" * (B + 6))[:3 * B + 17]))
    out.append(("period4", (b"abcd" * B)[:B + 1]))
    out.append(("second_block_repeats_first", noise[:B] * 2))           # the match across the boundary is not taken
    out.append(("one_literal_twice", b"\x41\x41"))                       # no match possible in 2 bytes
    counts = fibonacci(20)                                               # 17710 bytes; unlimited depth 19: the 15-bit limiter
    fib = np.concatenate([np.full(c, 11 * i + 3, np.uint8) for i, c in enumerate(counts)])
    rng.shuffle(fib)
    out.append(("fibonacci_counts", fib.tobytes()))
    out.append(("smooth_fixture", smooth_fixture()))
    t = np.arange(491520 // 4)
    clip = (2 ** 22 * np.sin(2 * np.pi * 700.0 * t / 12288.0) + rng.randn(t.size) * 2 ** 12).astype("<i4")
    out.append(("tone_plus_noise_int32", clip.tobytes()[:3 * B]))
    return out


class Planter(object):
    """One block of seeded noise with planted copies, so that its tokens are known by construction.  The parse takes a
    planted copy as planted when the source is candidate A of its first position: the LARGEST position of equal hash before
    the position's sub-step.  In a block of noise some later position often holds the same hash, so `place` checks exactly
    that with the restatement's hash, and moves the copy on by `step` until it holds.  `planted` lists what was placed:
    [(p, length, distance)].  Bytes before the copy stay as they are, except the one in front of it."""

    def __init__(self, rng, n):
        self.rng, self.n = rng, n
        self.b = rng.randint(0, 256, n).astype(np.uint8)
        self.h = ref.hashes(self.b)
        self.planted = []

    def _write(self, at, values):
        values = np.asarray(values, np.uint8)
        self.b[at:at + len(values)] = values
        lo, hi = max(at - 2, 0), min(at + len(values), self.n - 2)
        if hi > lo:
            self.h[lo:hi] = ref.hashes(self.b[lo:hi + 2])

    def candidate_a(self, p):
        """candidate A of p, or -1"""
        s = p - p % ref.CHUNK
        if p + 2 >= self.n or s == 0:
            return -1
        q = np.nonzero(self.h[:s] == self.h[p])[0]
        return int(q[-1]) if q.size else -1

    def match(self, q, p):
        m, cap = 0, min(ref.MAX_MATCH, self.n - p)
        while m < cap and self.b[q + m] == self.b[p + m]:
            m += 1
        return m

    def place(self, p, length, dist=None, src=None, step=1, front=None):
        """plant a copy of `length` bytes at the first p, p + step, ... where the parse takes it: from p - dist, or from
        the fixed position `src` (then any source that gives exactly `length` will do, an earlier copy of it for one);
        the bytes in front of and behind the copy are made to differ from the source's (`front`: the caller's byte
        for the one in front, which differs) -> p"""
        while True:
            q = p - dist if src is None else src
            assert q >= 0 and p + length <= self.n, (p, length, dist, src)
            keep = self.b[p - 1:p + length + 1].copy()
            if front is not None:
                self.b[p - 1] = front
            while q >= 1 and self.b[p - 1] == self.b[q - 1]:
                self.b[p - 1] = self.rng.randint(0, 256)
            for i in range(length):                                  # byte by byte: a source may overlap its copy
                self.b[p + i] = self.b[q + i]
            if p + length < self.n:
                while self.b[p + length] == self.b[q + length]:
                    self.b[p + length] = self.rng.randint(0, 256)
            self._write(p - 1, self.b[p - 1:p + length + 1].copy())
            a = self.candidate_a(p)
            if dist == 1 or (a >= 0 and self.match(a, p) == length and (src is not None or a == q)):
                self.planted.append((p, length, p - a if dist != 1 else 1))
                return p
            self._write(p - 1, keep)
            p += step

    def bytes(self):
        return self.b.tobytes()


DIST_BASE = {}                     # distance code -> its smallest distance, for the distances a block can hold
for _d in range(1, B):
    DIST_BASE.setdefault(ref.dist_code(_d)[0], _d)


def _every_length(rng):
    """Every match length 258 down to 3, over three blocks, each a copy of the head of a 259-byte pool at its block's
    start.  The lengths fall, so whichever earlier copy holds the hash is longer than the one being planted, and the byte
    behind the copy ends it at exactly its length; the bytes in front of the copies are distinct, so no match starts there."""
    blocks, length = [], 258
    while length >= 3:
        pl = Planter(rng, B)
        fronts = [v for v in rng.permutation(256) if v != pl.b[7]]
        at, k = 8 + 259 + 2, 0
        while length >= 3 and at + length + 4 <= B and k < len(fronts):
            p = pl.place(at, length, src=8, front=fronts[k])
            at, k, length = p + length + 2, k + 1, length - 1
        blocks.append(pl.bytes() if length >= 3 else pl.bytes()[:at])          # the last block is short
    return b"".join(blocks)


LARGEST_DISTANCE = B - 3           # a match has three bytes: it starts at B - 3 at the latest, its source at 0 at the earliest


def edge_distances():
    """1, 2, 3, 4 and the smallest and the largest distance of every distance code with extra bits that a block can hold"""
    top = max(DIST_BASE)
    return [1, 2, 3, 4] + [d for c in range(4, top + 1)
                           for d in (DIST_BASE[c], DIST_BASE[c + 1] - 1 if c < top else LARGEST_DISTANCE)]


def _every_distance_code(rng):
    """One block of exactly B bytes with a 3-byte copy at every distance of `edge_distances`, then a short last block.
    A distance below 256 is taken only from a source before the sub-step's start, so those copies stand at multiples of 256
    (distance 2 has only p % 256 in {0, 1}; 1 is a run, candidate B).  The largest distance a block can hold has its copy
    at B - 3 and its source at 0: the match that ends the block of exactly B bytes, cut by min(258, n - p).  The last
    block's last match is cut the same way, 100 bytes of a source that goes on."""
    pl = Planter(rng, B)
    for at in (600, 900, 1200):                        # three long copies make the block worth coding dynamic
        pl.place(at, 258, dist=400)
    at = 1536
    for d in edge_distances()[:-1]:
        if d < ref.CHUNK:
            p = pl.place(-(-at // ref.CHUNK) * ref.CHUNK, 3, dist=d, step=ref.CHUNK)
        else:
            p = pl.place(max(at, d + 8), 3, dist=d)
        at = p + 3 + 2
    assert at < B - 8
    while True:                          # the source at 0: draw its three bytes until no later position holds their hash
        pl._write(0, rng.randint(0, 256, 3))
        pl._write(B - 3, pl.b[:3].copy())
        if pl.candidate_a(B - 3) == 0:
            break
    last = Planter(rng, 700)
    last.place(600, 100, dist=300)
    return pl.bytes() + last.bytes()


# (length, distance) of the four rare long far copies: a length code with five extra bits each, used once; distance codes 26, 27
WIDE_FAR = ((231, 8198), (200, 12389), (150, 12300), (180, 8200))


def _wide_tokens(rng, lead):
    """One block: 3-byte copies at the smallest distances of the twelve distance codes 16..27, five times the Fibonacci
    numbers of them (the nearest the most), give a deep distance code; the long far copies of WIDE_FAR, whose length codes
    are used once, are then tokens of two long codes, 5 and 12 extra bits.  `lead` literals before the first of them move their
    bit offsets: 3 was found to put two of them at a shift of 29, from where they reach a third output word."""
    pl = Planter(rng, B)
    at = 600
    for code, count in zip(range(16, 28), reversed(fibonacci(12))):
        for _ in range(5 * count):
            at = pl.place(max(at, DIST_BASE[code] + 8), 3, dist=DIST_BASE[code]) + 3 + 2
    at = max(at, WIDE_FAR[1][1] + 8) + lead
    for length, dist in WIDE_FAR:
        at = pl.place(at, length, dist=dist) + length + 2
    return pl.bytes()[:at + 8]


def _smallest_hclen(rng):
    """One block whose code lengths all lie in 4..11: noise literals, and 10-byte copies at sixteen distance codes 12..27,
    eight of each, so the distance code is sixteen codes of 4 bits (a stray match may add a longer one)"""
    pl = Planter(rng, 14000)
    at = 600
    for code in range(12, 28):
        for _ in range(8):
            d = DIST_BASE[code] + 1
            if d < ref.CHUNK:
                p = pl.place(-(-at // ref.CHUNK) * ref.CHUNK, 10, dist=d, step=ref.CHUNK)
            else:
                p = pl.place(max(at, d + 8), 10, dist=d)
            at = p + 10 + 2
    return pl.bytes()[:at + 8]


def _one_distance_code(rng):
    """twenty 20-byte copies in 3000 bytes of noise, all at distance 300: distance code 16 alone, HDIST 17, one code of 1 bit"""
    pl = Planter(rng, 3000)
    for at in range(400, 2900, 125):
        pl.place(at, 20, dist=300)
    return pl.bytes()


def _noise_block_with_copy(seed, length):
    """B bytes of noise of `seed` with one copy of `length` bytes at distance 300: every byte copied saves about one byte"""
    pl = Planter(np.random.RandomState(seed), B)
    pl.place(5000, length, dist=300)
    return pl.bytes()


def distinct_trigram_order(rng, pool):
    """a seeded order of the bytes of `pool` in which no three consecutive bytes occur twice (and no byte three times in a
    row): every position of it is a literal, whatever the hash table holds, so its histogram is the pool's"""
    s = rng.permutation(np.asarray(pool, np.int64))
    seen = set()
    for i in range(2, len(s)):
        for _ in range(64):
            t = (int(s[i - 2]) << 16) | (int(s[i - 1]) << 8) | int(s[i])
            if t not in seen and not s[i] == s[i - 1] == s[i - 2]:
                break
            j = rng.randint(i + 1, len(s)) if i + 1 < len(s) else i
            s[i], s[j] = s[j], s[i]
        seen.add(t)
    return s.astype(np.uint8)


def _deep_literal_code(rng, ncommon, reps, rare_counts):
    """One block whose literal/length histogram is known exactly: `ncommon` byte values `reps` times each and rare values with
    the given counts, in an order without a repeated trigram (all literals), and three 258-byte copies spliced in at
    distance 400 (symbol 285 three times; they make the block worth coding dynamic).  With the end-of-block symbol the small
    counts are 1, 1, 2, 3, 5, 8, ...: a Fibonacci chain that hangs below the flat tree of the common values."""
    vals = rng.permutation(256)
    rare, common = vals[:len(rare_counts)], vals[len(rare_counts):len(rare_counts) + ncommon]
    data = distinct_trigram_order(rng, np.concatenate([np.repeat(common, reps)] + [np.full(c, v) for v, c in zip(rare, rare_counts)]))
    for at in (1000, 4258, 7516):
        data = np.concatenate([data[:at], data[at - 400:at - 400 + 258], data[at:]])
    assert len(data) <= B
    return data.tobytes()


def _planted_payloads():
    out = [("every_length", _every_length(np.random.RandomState(11))),
           ("every_distance_code", _every_distance_code(np.random.RandomState(12))),
           ("wide_tokens", _wide_tokens(np.random.RandomState(13), 3)),
           ("smallest_hclen", _smallest_hclen(np.random.RandomState(14))),
           ("one_distance_code", _one_distance_code(np.random.RandomState(15)))]
    # seeds and lengths found once by trying, the census holds them to what they were found for: noise of seed 100 with a
    # copy of 58 bytes has dyn_bytes == n + 5 (stored), with 59 bytes n + 4 (dynamic); both non-final, so their markers count
    out.append(("stored_or_dynamic_edge", _noise_block_with_copy(100, 58) + _noise_block_with_copy(100, 59) + b"last"))
    # noise of seed 121 with a 258-byte copy leaves 2 pad bits (the 5-byte marker), of seed 101 3 (the 4-byte marker)
    out.append(("pad_bits_2_then_3", _noise_block_with_copy(121, 258) + _noise_block_with_copy(101, 258) + b"last"))
    # 249 values 56 times each below a chain of 9: the deepest leaf is at exactly 15, no limiter; 100 values 145 times each
    # below a chain of 12: unlimited depth 16, the 15-bit limiter acts inside the block kernel.  Both send HCLEN 19.
    fib = fibonacci(13)
    out.append(("literal_code_depth_15", _deep_literal_code(np.random.RandomState(20), 249, 56, [1, 2] + fib[4:9])))
    out.append(("literal_code_limited", _deep_literal_code(np.random.RandomState(20), 100, 145, [1, 2] + fib[4:12])))
    return out


MILD = _payloads()                 # what the suite began with; the census' "before" column
PAYLOADS = MILD + _planted_payloads()
assert max(len(p) for name, p in PAYLOADS if name != "smooth_fixture") <= 3 * B + 17



def many_block_calls():
    """[(name, [payload])]: two calls with more blocks than the 1024 threads of deflate_offsets_kernel, which gives each
    thread ceil(nblocks / 1024) consecutive blocks.  1025 one-byte payloads: the first count at which a thread holds two.
    Then 2053 blocks, three to a thread: payloads of 1 to 3 bytes, and three compressible ones of 2, 2 and 4 blocks whose
    first blocks are number 2, number 1001 and the fourth from the end, so that each lies across two threads' blocks."""
    rng = np.random.RandomState(21)
    smooth = smooth_fixture()

    def small(count):
        return [rng.randint(0, 256, 1 + i % 3).astype(np.uint8).tobytes() for i in range(count)]

    mixed = small(2) + [smooth[:B + 1]] + small(997) + [(b"\x01\x7f\xfe" * B)[:2 * B]] + small(1046) + [smooth[5 * B:8 * B + 17]]
    return [("1025_of_one_byte", [bytes([i % 251]) for i in range(1025)]), ("2053_blocks_mixed", mixed)]


def block_runs(payloads):
    """(nblocks, blocks per thread of the offsets kernel, [(first block, last block)] of every payload)"""
    runs, at = [], 0
    for p in payloads:
        k = -(-len(p) // B)
        runs.append((at, at + k - 1))
        at += k
    return at, -(-at // 1024), runs


# (name, counts): the test puts them at scattered symbols of each alphabet
HISTOGRAMS = (("one_symbol", [7]), ("two_symbols", [3, 900]), ("all_equal", [5] * 19), ("fibonacci_9", fibonacci(9)),
              ("fibonacci_17", fibonacci(17)), ("fibonacci_19", fibonacci(19)), ("ties", [1, 1, 1, 2, 2, 3, 4, 4, 100, 100]))
ALPHABETS = ((286, 15), (30, 15), (19, 7))


def histogram_rows(nsym):
    """int32 [len(HISTOGRAMS) + 2][nsym]: every histogram's counts spread over the alphabet (stride 7 from symbol 1,
    wrapped: 7 is coprime to 286, 30 and 19), then one row with every symbol used once and one with none used"""
    rows = np.zeros((len(HISTOGRAMS) + 2, nsym), np.int32)
    for r, (_, counts) in enumerate(HISTOGRAMS):
        for k, c in enumerate(counts):
            s = (1 + 7 * k) % nsym
            assert rows[r, s] == 0
            rows[r, s] = c
    rows[len(HISTOGRAMS)] = 1
    return rows


def check_lengths(freq, lengths, limit, what):
    """the properties every code must have: 0 exactly for unused symbols, lengths 1..limit, Kraft sum exactly 1 with two or
    more used symbols, and the cost of a heapq Huffman build whenever that build's depth fits the limit"""
    freq, lengths = [int(f) for f in freq], [int(l) for l in lengths]
    used = [i for i, f in enumerate(freq) if f > 0]
    for i, (f, l) in enumerate(zip(freq, lengths)):
        assert (1 <= l <= limit) if f > 0 else l == 0, (what, i, f, l)
    if len(used) == 1:
        assert lengths[used[0]] == 1, what
    if len(used) >= 2:
        assert sum(1 << (limit - lengths[i]) for i in used) == 1 << limit, (what, "Kraft sum")
        cost, depth = ref.heap_huffman_cost(freq)
        if depth <= limit:
            assert sum(freq[i] * lengths[i] for i in used) == cost, (what, "cost")
        return depth
    return len(used)
